"""ctypes binding of gr-fosphor_amd/libfosphor_amd.so (the C ABI of include/fosphor.h,
include/fosphor_amd.h and the headers beside them).  No CPU fallback: a missing library is a hard error."""
import ctypes as C
import os
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
# FOSPHOR_AMD_LIB lets the tuning harness (tools/ab_bench.sh) point at an alternative build
LIB_PATH = os.environ.get("FOSPHOR_AMD_LIB") or os.path.join(PKG_DIR, "libfosphor_amd.so")


class Config(C.Structure):
    """struct fosphor_amd_config (include/fosphor_amd.h)"""
    _fields_ = [("fft_len_log", C.c_int), ("n_bins", C.c_int), ("wf_rows", C.c_int),
                ("t0r", C.c_float), ("t0d", C.c_float), ("alpha", C.c_float),
                ("device", C.c_int), ("max_spectra", C.c_int), ("max_batches", C.c_int),
                ("stream", C.c_void_p), ("iq_format", C.c_int)]


class Buffers(C.Structure):
    """struct fosphor_amd_buffers"""
    _fields_ = [("d_waterfall", C.c_void_p), ("d_histogram", C.c_void_p), ("d_spectrum", C.c_void_p),
                ("d_hitcount", C.c_void_p), ("waterfall_pos", C.c_int),
                ("fft_len", C.c_int), ("n_bins", C.c_int), ("wf_rows", C.c_int),
                ("histo_scale", C.c_float), ("histo_offset", C.c_float)]


class Partials(C.Structure):
    """struct fosphor_amd_partials"""
    _fields_ = [("d_hc", C.c_void_p), ("d_live_sum", C.c_void_p), ("d_max", C.c_void_p),
                ("n_hc", C.c_int), ("n_cols", C.c_int)]


class CountPlan(C.Structure):
    """struct fosphor_amd_count_plan"""
    _fields_ = [("chunk", C.c_int), ("cpb", C.c_int), ("handoff", C.c_int), ("two_sets", C.c_int), ("rowmask", C.c_int),
                ("table", C.c_int), ("merge_form", C.c_int), ("table_in_memory", C.c_int)]


class K1Plan(C.Structure):
    """struct fosphor_amd_k1_plan"""
    _fields_ = [("kernel", C.c_int), ("tile", C.c_int), ("tiles", C.c_int), ("units", C.c_int), ("max_tiles", C.c_int),
                ("min_tiles", C.c_int)]


class Channel(C.Structure):
    _fields_ = [("enabled", C.c_int), ("center", C.c_float), ("width", C.c_float)]


class Render(C.Structure):
    """struct fosphor_render (include/fosphor.h; layout of the reference's fosphor.h:58-90)"""
    _fields_ = [("pos_x", C.c_int), ("pos_y", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("options", C.c_int), ("histo_wf_ratio", C.c_float), ("freq_n_div", C.c_int),
                ("freq_center", C.c_float), ("freq_span", C.c_float), ("wf_span", C.c_float),
                ("channels", Channel * 8),
                ("_wf_pos", C.c_int), ("_x_div", C.c_float), ("_x", C.c_float * 2), ("_x_label", C.c_float),
                ("_y_histo_div", C.c_float), ("_y_histo", C.c_float * 2), ("_y_wf", C.c_float * 2),
                ("_y_label", C.c_float)]


# every exported entry point: name -> (restype, argtypes)
class FreqAxis(C.Structure):
    """struct fosphor_amd_freq_axis (= the reference's struct freq_axis, axis.h:20-30)"""
    _fields_ = [("center", C.c_double), ("span", C.c_double), ("step", C.c_double), ("mode", C.c_int),
                ("abs_fmt", C.c_char * 16), ("abs_scale", C.c_double), ("rel_fmt", C.c_char * 16),
                ("rel_step", C.c_double)]


class View(C.Structure):
    """struct fosphor_amd_view (include/fosphor_amd_view.h)"""
    _fields_ = [("first_bin", C.c_int), ("n_cols", C.c_int), ("width", C.c_int),
                ("wf_src_rows", C.c_int), ("wf_out_rows", C.c_int), ("detector", C.c_int)]


class ViewColor(C.Structure):
    """struct fosphor_amd_view_color"""
    _fields_ = [("palette", C.c_void_p), ("n", C.c_int), ("use_defaults", C.c_int),
                ("scale", C.c_float), ("offset", C.c_float)]


class ViewOut(C.Structure):
    """struct fosphor_amd_view_out"""
    _fields_ = [("d_waterfall", C.c_void_p), ("d_histogram", C.c_void_p), ("d_live", C.c_void_p), ("d_max", C.c_void_p),
                ("d_waterfall_rgba", C.c_void_p), ("d_histogram_rgba", C.c_void_p),
                ("wf_color", ViewColor), ("histo_color", ViewColor)]


class DetectCfg(C.Structure):
    """struct fosphor_amd_detect_cfg (include/fosphor_amd_detect.h)"""
    _fields_ = [("trace", C.c_int), ("first_bin", C.c_int), ("n_cols", C.c_int), ("floor_mode", C.c_int),
                ("floor_q", C.c_float), ("margin_y", C.c_float), ("threshold_y", C.c_float),
                ("max_gap", C.c_int), ("min_cols", C.c_int)]


class DetectResult(C.Structure):
    """struct fosphor_amd_detect_result"""
    _fields_ = [("n_found", C.c_int32), ("n_written", C.c_int32), ("floor_bin", C.c_int32),
                ("floor_y", C.c_float), ("threshold_y", C.c_float)]


class Band(C.Structure):
    """struct fosphor_amd_band"""
    _fields_ = [("first", C.c_int32), ("last", C.c_int32), ("peak_col", C.c_int32),
                ("peak_y", C.c_float), ("power_y", C.c_float)]


class MaskChannel(C.Structure):
    """struct fosphor_amd_mask_channel (include/fosphor_amd_mask.h)"""
    _fields_ = [("first", C.c_int32), ("last", C.c_int32)]


class MaskCfg(C.Structure):
    """struct fosphor_amd_mask_cfg"""
    _fields_ = [("first_bin", C.c_int), ("n_cols", C.c_int), ("rows", C.c_int), ("min_cols", C.c_int),
                ("n_channels", C.c_int), ("channels", MaskChannel * 8)]


class MaskRow(C.Structure):
    """struct fosphor_amd_mask_row"""
    _fields_ = [("n_over", C.c_int32), ("n_under", C.c_int32), ("first_col", C.c_int32), ("last_col", C.c_int32),
                ("peak_col", C.c_int32), ("peak_over", C.c_float)]


class MaskResult(C.Structure):
    """struct fosphor_amd_mask_result"""
    _fields_ = [("n_triggered", C.c_int32), ("n_written", C.c_int32), ("newest", C.c_int32), ("oldest", C.c_int32)]


class BurstCfg(C.Structure):
    """struct fosphor_amd_burst_cfg (include/fosphor_amd_burst.h)"""
    _fields_ = [("first_bin", C.c_int), ("n_cols", C.c_int), ("rows", C.c_int), ("threshold_y", C.c_float),
                ("max_gap_cols", C.c_int), ("max_gap_rows", C.c_int), ("min_rows", C.c_int), ("min_cols", C.c_int),
                ("max_runs", C.c_int)]


class Burst(C.Structure):
    """struct fosphor_amd_burst"""
    _fields_ = [("newest", C.c_int32), ("oldest", C.c_int32), ("first_col", C.c_int32), ("last_col", C.c_int32),
                ("n_cells", C.c_int32), ("peak_row", C.c_int32), ("peak_col", C.c_int32), ("peak_y", C.c_float),
                ("energy_y", C.c_float), ("flags", C.c_uint32)]


class BurstResult(C.Structure):
    """struct fosphor_amd_burst_result"""
    _fields_ = [("n_runs", C.c_int32), ("n_components", C.c_int32), ("n_found", C.c_int32), ("n_written", C.c_int32),
                ("overflow", C.c_int32)]


class ExtractJob(C.Structure):
    """struct fosphor_amd_extract_job (include/fosphor_amd_extract.h)"""
    _fields_ = [("first", C.c_int64), ("out_offset", C.c_int64), ("n_out", C.c_int32), ("decim", C.c_int32),
                ("phase_inc", C.c_uint32), ("phase0", C.c_uint32), ("taps_offset", C.c_int32), ("n_taps", C.c_int32)]


class MeasureJob(C.Structure):
    """struct fosphor_amd_measure_job (include/fosphor_amd_measure.h)"""
    _fields_ = [("offset", C.c_int64), ("n", C.c_int32), ("threshold", C.c_float)]


class DemodJob(C.Structure):
    """struct fosphor_amd_demod_job (include/fosphor_amd_demod.h)"""
    _fields_ = [("offset", C.c_int64), ("out_offset", C.c_int64), ("n", C.c_int32), ("mode", C.c_int32), ("avg", C.c_int32),
                ("reserved", C.c_int32)]


class CorrelateJob(C.Structure):
    """struct fosphor_amd_correlate_job (include/fosphor_amd_correlate.h)"""
    _fields_ = [("offset", C.c_int64), ("out_offset", C.c_int64), ("tpl_offset", C.c_int64), ("n", C.c_int32),
                ("tpl_len", C.c_int32), ("trace", C.c_int32), ("threshold", C.c_float)]


class CorrelateRecord(C.Structure):
    """struct fosphor_amd_correlate_record"""
    _fields_ = [("n_lags", C.c_int32), ("n_above", C.c_int32), ("first_above", C.c_int32), ("last_above", C.c_int32),
                ("n_edges", C.c_int32), ("peak_lag", C.c_int32), ("peak_rho", C.c_float), ("tpl_len", C.c_int32),
                ("peak_c_re", C.c_double), ("peak_c_im", C.c_double), ("peak_energy", C.c_double), ("tpl_energy", C.c_double)]


class CorrelateValues(C.Structure):
    """struct fosphor_amd_correlate_values"""
    _fields_ = [(k, C.c_double) for k in ("time", "rho", "gain_re", "gain_im", "gain_db", "phase_turns", "snr_db", "detections")]


class PsdJob(C.Structure):
    """struct fosphor_amd_psd_job (include/fosphor_amd_psd.h)"""
    _fields_ = [("offset", C.c_int64), ("out_offset", C.c_int64), ("win_offset", C.c_int64), ("n", C.c_int32),
                ("fft_len_log", C.c_int32), ("hop", C.c_int32), ("pre", C.c_int32), ("trace", C.c_int32),
                ("obw_fraction", C.c_float), ("xdb_ratio", C.c_float), ("reserved", C.c_int32)]


class PsdRecord(C.Structure):
    """struct fosphor_amd_psd_record"""
    _fields_ = [("n_seg", C.c_int32), ("fft_len", C.c_int32), ("peak_bin", C.c_int32), ("peak_power", C.c_float),
                ("obw_lo", C.c_int32), ("obw_hi", C.c_int32), ("xdb_lo", C.c_int32), ("xdb_hi", C.c_int32),
                ("total", C.c_double), ("m1", C.c_double), ("m2", C.c_double), ("win_energy", C.c_double)]


class PsdValues(C.Structure):
    """struct fosphor_amd_psd_values"""
    _fields_ = [(k, C.c_double) for k in ("mean_power", "peak_freq", "peak_db", "centroid", "rms_width", "obw", "obw_centre",
                                          "xdb_bandwidth")]


class SymbolsJob(C.Structure):
    """struct fosphor_amd_symbols_job (include/fosphor_amd_symbols.h)"""
    _fields_ = [("offset", C.c_int64), ("out_offset", C.c_int64), ("n", C.c_int32), ("sps", C.c_int32), ("mode", C.c_int32),
                ("tau", C.c_float), ("reserved", C.c_int32 * 2)]


class SymbolsRecord(C.Structure):
    """struct fosphor_amd_symbols_record"""
    _fields_ = [("n_sym", C.c_int32), ("first", C.c_int32), ("tau", C.c_float), ("status", C.c_int32), ("mu", C.c_double),
                ("x_re", C.c_double), ("x_im", C.c_double), ("a0", C.c_double), ("m2", C.c_double), ("m4", C.c_double),
                ("z2_re", C.c_double), ("z2_im", C.c_double), ("z4_re", C.c_double), ("z4_im", C.c_double)]


class SymbolsValues(C.Structure):
    """struct fosphor_amd_symbols_values"""
    _fields_ = [(k, C.c_double) for k in ("tau", "t_first", "symbol_rate", "timing_depth", "sym_power", "snr_db", "phase2", "lock2",
                                          "phase4", "lock4")]


class CarrierJob(C.Structure):
    """struct fosphor_amd_carrier_job (include/fosphor_amd_carrier.h)"""
    _fields_ = [("offset", C.c_int64), ("out_offset", C.c_int64), ("n", C.c_int32), ("order", C.c_int32), ("mode", C.c_int32),
                ("lag", C.c_int32), ("freq", C.c_double), ("phase", C.c_double)]


class CarrierRecord(C.Structure):
    """struct fosphor_amd_carrier_record"""
    _fields_ = [("n", C.c_int32), ("order", C.c_int32), ("lag_used", C.c_int32), ("status", C.c_int32), ("freq", C.c_double),
                ("phase", C.c_double), ("r1_re", C.c_double), ("r1_im", C.c_double), ("rl_re", C.c_double), ("rl_im", C.c_double),
                ("z_re", C.c_double), ("z_im", C.c_double), ("m2", C.c_double), ("mm", C.c_double)]


class CarrierValues(C.Structure):
    """struct fosphor_amd_carrier_values"""
    _fields_ = [(k, C.c_double) for k in ("freq_hz", "phase_rad", "sym_power", "lock", "lag_lock", "lagl_lock")]


class DecideJob(C.Structure):
    """struct fosphor_amd_decide_job (include/fosphor_amd_decide.h)"""
    _fields_ = [("offset", C.c_int64), ("out_offset", C.c_int64), ("n", C.c_int32), ("order", C.c_int32), ("flags", C.c_int32),
                ("uw_offset", C.c_int32), ("uw_len", C.c_int32), ("uw_first", C.c_int32), ("uw_count", C.c_int32),
                ("uw_max_errors", C.c_int32), ("reserved", C.c_int32 * 4)]


class DecideRecord(C.Structure):
    """struct fosphor_amd_decide_record"""
    _fields_ = [("n", C.c_int32), ("order", C.c_int32), ("flags", C.c_int32), ("status", C.c_int32), ("uw_pos", C.c_int32),
                ("uw_rot", C.c_int32), ("uw_errors", C.c_int32), ("erasures", C.c_int32), ("a", C.c_double), ("b", C.c_double),
                ("m2", C.c_double), ("hist", C.c_int32 * 8), ("reserved", C.c_int32 * 2)]


class DecideValues(C.Structure):
    """struct fosphor_amd_decide_values"""
    _fields_ = [(k, C.c_double) for k in ("gain", "evm_rms", "mer_db", "phase_err_rad", "uw_error_rate")]


class DecodeJob(C.Structure):
    """struct fosphor_amd_decode_job (include/fosphor_amd_decode.h)"""
    _fields_ = [("offset", C.c_int64), ("out_offset", C.c_int64), ("n", C.c_int32), ("order", C.c_int32), ("steps", C.c_int32),
                ("flags", C.c_int32), ("k", C.c_uint8), ("n_poly", C.c_uint8), ("period", C.c_uint8), ("crc_width", C.c_uint8),
                ("polys", C.c_uint16 * 3), ("punct", C.c_uint16 * 3), ("crc_poly", C.c_uint32), ("crc_init", C.c_uint32),
                ("crc_xorout", C.c_uint32), ("reserved", C.c_uint32)]


class DecodeRecord(C.Structure):
    """struct fosphor_amd_decode_record"""
    _fields_ = [("n_steps", C.c_int32), ("n_bits", C.c_int32), ("n_coded", C.c_int32), ("status", C.c_int32),
                ("end_state", C.c_int32), ("metric", C.c_int32), ("best_state", C.c_int32), ("best_metric", C.c_int32),
                ("crc_calc", C.c_uint32), ("crc_recv", C.c_uint32), ("k", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class DecodeValues(C.Structure):
    """struct fosphor_amd_decode_values"""
    _fields_ = [(k, C.c_double) for k in ("channel_ber", "rate", "crc_ok")]


class SoftJob(C.Structure):
    """struct fosphor_amd_soft_job (include/fosphor_amd_soft.h)"""
    _fields_ = [("offset", C.c_int64), ("out_offset", C.c_int64), ("n", C.c_int32), ("order", C.c_int16), ("flags", C.c_int16),
                ("steps", C.c_int32), ("k", C.c_uint8), ("n_poly", C.c_uint8), ("period", C.c_uint8), ("crc_width", C.c_uint8),
                ("polys", C.c_uint16 * 3), ("punct", C.c_uint16 * 3), ("crc_poly", C.c_uint32), ("crc_init", C.c_uint32),
                ("crc_xorout", C.c_uint32), ("rot", C.c_int32), ("scale", C.c_float)]


class SoftRecord(C.Structure):
    """struct fosphor_amd_soft_record"""
    _fields_ = [("n_steps", C.c_int32), ("n_bits", C.c_int32), ("n_coded", C.c_int32), ("status", C.c_int32),
                ("end_state", C.c_int32), ("metric", C.c_int32), ("best_state", C.c_int32), ("best_metric", C.c_int32),
                ("crc_calc", C.c_uint32), ("crc_recv", C.c_uint32), ("k", C.c_int32), ("flags", C.c_int32),
                ("erasures", C.c_int32), ("saturated", C.c_int32), ("abs_sum", C.c_int64)]


class SoftValues(C.Structure):
    """struct fosphor_amd_soft_values"""
    _fields_ = [(k, C.c_double) for k in ("mean_abs", "corrected_share", "rate", "crc_ok")]


class RsJob(C.Structure):
    """struct fosphor_amd_rs_job (include/fosphor_amd_rs.h)"""
    _fields_ = [("offset", C.c_int64), ("out_offset", C.c_int64), ("flags", C.c_int32), ("gf_poly", C.c_uint16), ("fcr", C.c_uint8),
                ("prim", C.c_uint8), ("n_roots", C.c_uint8), ("n_code", C.c_uint8), ("depth", C.c_uint8), ("scr_width", C.c_uint8),
                ("scr_taps", C.c_uint32), ("scr_init", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class RsRecord(C.Structure):
    """struct fosphor_amd_rs_record"""
    _fields_ = [("n_codewords", C.c_int32), ("n_data", C.c_int32), ("status", C.c_int32), ("n_failed", C.c_int32),
                ("n_clean", C.c_int32), ("corrected_symbols", C.c_int32), ("corrected_bits", C.c_int32), ("max_errors", C.c_int32),
                ("failed_mask", C.c_uint32), ("errors", C.c_uint8 * 16), ("n_code", C.c_uint16), ("n_roots", C.c_uint16),
                ("reserved", C.c_uint32 * 2)]


class RsValues(C.Structure):
    """struct fosphor_amd_rs_values"""
    _fields_ = [(k, C.c_double) for k in ("byte_error_rate", "failed_share", "ok")]


class ResampleJob(C.Structure):
    """struct fosphor_amd_resample_job (include/fosphor_amd_resample.h)"""
    _fields_ = [("offset", C.c_int64), ("out_offset", C.c_int64), ("phase0", C.c_int64), ("n", C.c_int32), ("n_out", C.c_int32),
                ("up", C.c_int32), ("down", C.c_int32), ("taps_offset", C.c_int32), ("n_taps", C.c_int32)]


class MeasureValues(C.Structure):
    """struct fosphor_amd_measure_values"""
    _fields_ = [(k, C.c_double) for k in ("mean_power", "mean_db", "peak_db", "papr_db", "freq_offset", "coherence", "kurtosis",
                                          "circularity", "dc_fraction", "duty", "rise", "fall", "pulses")]


class Wire(C.Structure):
    """struct fosphor_amd_wire (include/fosphor_amd_wire.h)"""
    _fields_ = [("d_masks", C.c_void_p), ("mask_words", C.c_int), ("world", C.c_int), ("d_words", C.c_void_p),
                ("n_words", C.c_int), ("form", C.c_int), ("live_rows", C.c_int), ("rows", C.c_int)]


SIGNATURES = {
    # include/fosphor.h
    "fosphor_init": (C.c_void_p, []),
    "fosphor_release": (None, [C.c_void_p]),
    "fosphor_process": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fosphor_draw": (None, [C.c_void_p, C.POINTER(Render)]),
    "fosphor_set_fft_window_default": (None, [C.c_void_p]),
    "fosphor_set_fft_window": (None, [C.c_void_p, C.c_void_p]),
    "fosphor_set_power_range": (None, [C.c_void_p, C.c_int, C.c_int]),
    "fosphor_set_frequency_range": (None, [C.c_void_p, C.c_double, C.c_double]),
    "fosphor_render_defaults": (None, [C.POINTER(Render)]),
    "fosphor_render_refresh": (None, [C.POINTER(Render)]),
    "fosphor_pos2freq": (C.c_double, [C.c_void_p, C.POINTER(Render), C.c_int]),
    "fosphor_pos2pwr": (C.c_float, [C.c_void_p, C.POINTER(Render), C.c_int]),
    "fosphor_pos2samp": (C.c_int, [C.c_void_p, C.POINTER(Render), C.c_int]),
    "fosphor_freq2pos": (C.c_int, [C.c_void_p, C.POINTER(Render), C.c_double]),
    "fosphor_pwr2pos": (C.c_int, [C.c_void_p, C.POINTER(Render), C.c_float]),
    "fosphor_samp2pos": (C.c_int, [C.c_void_p, C.POINTER(Render), C.c_int]),
    "fosphor_render_pos_inside": (C.c_int, [C.POINTER(Render), C.c_int, C.c_int]),
    # include/fosphor_amd.h
    "fosphor_amd_init": (C.c_void_p, [C.POINTER(Config)]),
    "fosphor_amd_process_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "fosphor_amd_process_device_overlap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fosphor_amd_finish": (C.c_int, [C.c_void_p]),
    "fosphor_amd_get_buffers": (C.c_int, [C.c_void_p, C.POINTER(Buffers)]),
    "fosphor_amd_get_buffers_nohc": (C.c_int, [C.c_void_p, C.POINTER(Buffers)]),
    "fosphor_amd_read": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]),
    "fosphor_amd_fft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fosphor_amd_bin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fosphor_amd_accumulate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fosphor_amd_accumulate_device_overlap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fosphor_amd_set_partial_slot": (C.c_int, [C.c_void_p, C.c_int]),
    "fosphor_amd_get_partials": (C.c_int, [C.c_void_p, C.POINTER(Partials)]),
    "fosphor_amd_merge": (C.c_int, [C.c_void_p, C.c_int]),
    "fosphor_amd_comm_unique_id": (C.c_int, [C.c_void_p]),
    "fosphor_amd_comm_init": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p]),
    "fosphor_amd_comm_destroy": (C.c_int, [C.c_void_p]),
    "fosphor_amd_comm_available": (C.c_int, []),
    "fosphor_amd_comm_count": (C.c_int, [C.c_void_p]),
    "fosphor_amd_exchange_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "fosphor_amd_exchange": (C.c_int, [C.c_void_p, C.c_void_p]),
    "fosphor_amd_exchange_sliced": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "fosphor_amd_merge_sliced": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fosphor_amd_gather_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "fosphor_amd_profile": (None, [C.c_void_p, C.c_int]),
    "fosphor_amd_kernel_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float * 3), C.POINTER(C.c_int * 3)]),
    "fosphor_amd_kernel_busy": (C.c_int, [C.c_void_p, C.POINTER(C.c_float * 3)]),
    "fosphor_amd_host_thresholds": (C.c_int, [C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "fosphor_amd_host_twiddle_count": (C.c_int, []),
    "fosphor_amd_host_twiddles": (C.c_int, [C.c_void_p]),
    "fosphor_amd_set_overlap": (C.c_int, [C.c_void_p, C.c_int]),
    "fosphor_amd_traffic_twin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "fosphor_amd_set_input_ordering": (C.c_int, [C.c_void_p, C.c_int]),
    "fosphor_amd_wait_input": (C.c_int, [C.c_void_p]),
    "fosphor_amd_stream": (C.c_void_p, [C.c_void_p]),
    "fosphor_amd_stream2": (C.c_void_p, [C.c_void_p]),
    "fosphor_amd_upload_stream": (C.c_void_p, [C.c_void_p]),
    "fosphor_amd_tune_placement": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "fosphor_amd_plan_piece_batches": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong]),
    "fosphor_amd_plan_count": (C.c_int, [C.c_int] * 8 + [C.POINTER(CountPlan)]),
    "fosphor_amd_plan_k1": (C.c_int, [C.c_int] * 10 + [C.POINTER(K1Plan)]),
    "fosphor_amd_share_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "fosphor_amd_launch_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "fosphor_amd_merge_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 11)]),
    "fosphor_amd_version": (C.c_char_p, []),
    # include/fosphor_amd_axis.h
    "fosphor_amd_freq_axis_build": (None, [C.c_void_p, C.c_double, C.c_double, C.c_int]),
    "fosphor_amd_freq_axis_render": (None, [C.c_void_p, C.c_char_p, C.c_int]),
    "fosphor_amd_freq_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fosphor_amd_power_labels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int * 11)]),
    # include/fosphor_amd_cmap.h
    "fosphor_amd_cmap_generate": (C.c_int, [C.c_int, C.c_void_p, C.c_int]),
    "fosphor_amd_colorize": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float,
                                       C.c_int, C.c_void_p]),
    # include/fosphor_amd_view.h
    "fosphor_amd_view": (C.c_int, [C.c_void_p, C.POINTER(View), C.POINTER(ViewOut)]),
    "fosphor_amd_view_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 4)]),
    "fosphor_amd_view_span": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fosphor_amd_view_from_render": (C.c_int, [C.c_int, C.c_int, C.POINTER(Render), C.c_int, C.c_int, C.POINTER(View)]),
    # include/fosphor_amd_detect.h
    "fosphor_amd_percentiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fosphor_amd_detect": (C.c_int, [C.c_void_p, C.POINTER(DetectCfg), C.c_void_p, C.c_void_p, C.c_int]),
    "fosphor_amd_detect_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 3)]),
    "fosphor_amd_detect_bin_y": (C.c_int, [C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "fosphor_amd_detect_bands_host": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                C.POINTER(C.c_int)]),
    # include/fosphor_amd_mask.h
    "fosphor_amd_mask_scan": (C.c_int, [C.c_void_p, C.POINTER(MaskCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_void_p]),
    "fosphor_amd_mask_from_trace": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "fosphor_amd_mask_from_points": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "fosphor_amd_mask_row_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(MaskRow)]),
    "fosphor_amd_mask_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 4)]),
    # include/fosphor_amd_burst.h
    "fosphor_amd_bursts": (C.c_int, [C.c_void_p, C.POINTER(BurstCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fosphor_amd_bursts_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(BurstCfg), C.POINTER(BurstResult),
                                          C.c_void_p, C.c_int]),
    "fosphor_amd_burst_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 10)]),
    # include/fosphor_amd_extract.h
    "fosphor_amd_extract": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int64]),
    "fosphor_amd_extract_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_int64]),
    "fosphor_amd_extract_design": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_void_p]),
    "fosphor_amd_extract_from_burst": (C.c_int, [C.POINTER(Burst), C.c_int, C.c_int64, C.c_int, C.c_int, C.c_double,
                                                 C.POINTER(ExtractJob), C.POINTER(C.c_int)]),
    "fosphor_amd_extract_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 6)]),
    # include/fosphor_amd_measure.h
    "fosphor_amd_measure": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
    "fosphor_amd_measure_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
    "fosphor_amd_measure_from_extract": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(MeasureJob)]),
    "fosphor_amd_measure_derive": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(MeasureValues)]),
    "fosphor_amd_measure_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 7)]),
    # include/fosphor_amd_demod.h
    "fosphor_amd_demod": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    "fosphor_amd_demod_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    "fosphor_amd_demod_n_out": (C.c_int, [C.c_int, C.c_int32, C.c_int]),
    "fosphor_amd_demod_from_extract": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(DemodJob)]),
    "fosphor_amd_demod_atan2_turns": (C.c_float, [C.c_double, C.c_double]),
    "fosphor_amd_demod_atan2_turns_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "fosphor_amd_demod_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 7)]),
    # include/fosphor_amd_correlate.h
    "fosphor_amd_correlate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_int64]),
    "fosphor_amd_correlate_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_int64]),
    "fosphor_amd_correlate_n_out": (C.c_int, [C.c_int, C.c_int32, C.c_int]),
    "fosphor_amd_correlate_from_extract": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.POINTER(CorrelateJob)]),
    "fosphor_amd_correlate_derive": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(CorrelateValues)]),
    "fosphor_amd_correlate_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 6)]),
    # include/fosphor_amd_resample.h
    "fosphor_amd_resample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_int64]),
    "fosphor_amd_resample_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_int64]),
    "fosphor_amd_resample_n_out": (C.c_int, [C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int64]),
    "fosphor_amd_resample_design": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]),
    "fosphor_amd_resample_ratio": (C.c_int, [C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                             C.POINTER(C.c_double)]),
    "fosphor_amd_resample_from_extract": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(ResampleJob)]),
    "fosphor_amd_resample_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 7)]),
    # include/fosphor_amd_psd.h
    "fosphor_amd_psd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_int64]),
    "fosphor_amd_psd_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_int64]),
    "fosphor_amd_psd_n_seg": (C.c_int, [C.c_int32, C.c_int, C.c_int]),
    "fosphor_amd_psd_window": (C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    "fosphor_amd_psd_twiddles": (C.c_int, [C.c_void_p]),
    "fosphor_amd_psd_from_extract": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                               C.POINTER(PsdJob)]),
    "fosphor_amd_psd_ratio_from_db": (C.c_double, [C.c_double]),
    "fosphor_amd_psd_derive": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(PsdValues)]),
    "fosphor_amd_psd_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 6)]),
    # include/fosphor_amd_symbols.h
    "fosphor_amd_symbols": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "fosphor_amd_symbols_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "fosphor_amd_symbols_max_out": (C.c_int, [C.c_int32, C.c_int]),
    "fosphor_amd_symbols_twiddles": (C.c_int, [C.c_int, C.c_void_p]),
    "fosphor_amd_symbols_from_extract": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(SymbolsJob)]),
    "fosphor_amd_symbols_from_resample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.POINTER(SymbolsJob)]),
    "fosphor_amd_symbols_derive": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.POINTER(SymbolsValues)]),
    "fosphor_amd_symbols_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 9)]),
    # include/fosphor_amd_carrier.h
    "fosphor_amd_carrier": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "fosphor_amd_carrier_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "fosphor_amd_carrier_from_symbols": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                                   C.POINTER(CarrierJob)]),
    "fosphor_amd_carrier_derive": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(CarrierValues)]),
    "fosphor_amd_carrier_cossin_turns": (C.c_int, [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "fosphor_amd_carrier_cossin_turns_n": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "fosphor_amd_carrier_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 9)]),
    # include/fosphor_amd_decide.h
    "fosphor_amd_decide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_int64]),
    "fosphor_amd_decide_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_int64]),
    "fosphor_amd_decide_from_carrier": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(DecideJob)]),
    "fosphor_amd_decide_derive": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(DecideValues)]),
    "fosphor_amd_decide_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 7)]),
    # include/fosphor_amd_decode.h
    "fosphor_amd_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "fosphor_amd_decode_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "fosphor_amd_decode_steps": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "fosphor_amd_decode_from_decide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(DecodeJob)]),
    "fosphor_amd_decode_derive": (C.c_int, [C.c_void_p, C.POINTER(DecodeValues)]),
    "fosphor_amd_decode_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 7)]),
    # include/fosphor_amd_soft.h
    "fosphor_amd_soft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "fosphor_amd_soft_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "fosphor_amd_soft_from_decide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(SoftJob)]),
    "fosphor_amd_soft_derive": (C.c_int, [C.c_void_p, C.POINTER(SoftValues)]),
    "fosphor_amd_soft_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 7)]),
    # include/fosphor_amd_rs.h
    "fosphor_amd_rs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "fosphor_amd_rs_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "fosphor_amd_rs_encode_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    "fosphor_amd_rs_from_decode": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_int, C.c_int, C.POINTER(RsJob)]),
    "fosphor_amd_rs_derive": (C.c_int, [C.c_void_p, C.POINTER(RsValues)]),
    "fosphor_amd_rs_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 8)]),
    # include/fosphor_amd_wire.h
    "fosphor_amd_wire_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fosphor_amd_wire_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Wire)]),
    "fosphor_amd_wire_unpack": (C.c_int, [C.c_void_p]),
    "fosphor_amd_wire_get": (C.c_int, [C.c_void_p, C.POINTER(Wire)]),
    "fosphor_amd_exchange_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fosphor_amd_wire_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong * 5)]),
    "fosphor_amd_wire_kernel_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float * 3)]),
    # include/fosphor_amd_sink.h
    "fosphor_amd_process_pinned": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fosphor_amd_upload_pinned": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fosphor_amd_process_uploaded": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "fosphor_amd_pending_uploads": (C.c_int, [C.c_void_p]),
    "fosphor_amd_wait_upload": (C.c_int, [C.c_void_p]),
    "fosphor_amd_fifo_new": (C.c_void_p, [C.c_int, C.c_int]),
    "fosphor_amd_fifo_free": (None, [C.c_void_p]),
    "fosphor_amd_fifo_free_space": (C.c_int, [C.c_void_p]),
    "fosphor_amd_fifo_used": (C.c_int, [C.c_void_p]),
    "fosphor_amd_fifo_write_max_size": (C.c_int, [C.c_void_p]),
    "fosphor_amd_fifo_write_prepare": (C.c_void_p, [C.c_void_p, C.c_int, C.c_int]),
    "fosphor_amd_fifo_write_commit": (None, [C.c_void_p, C.c_int]),
    "fosphor_amd_fifo_read_max_size": (C.c_int, [C.c_void_p]),
    "fosphor_amd_fifo_read_peek": (C.c_void_p, [C.c_void_p, C.c_int, C.c_int]),
    "fosphor_amd_fifo_read_discard": (None, [C.c_void_p, C.c_int]),
    "fosphor_amd_sink_new": (C.c_void_p, []),
    "fosphor_amd_sink_new_len": (C.c_void_p, [C.c_int]),
    "fosphor_amd_sink_feed": (C.c_double, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fosphor_amd_sink_free": (None, [C.c_void_p]),
    "fosphor_amd_sink_dropped": (C.c_uint64, [C.c_void_p]),
    "fosphor_amd_sink_start": (C.c_int, [C.c_void_p]),
    "fosphor_amd_sink_stop": (C.c_int, [C.c_void_p]),
    "fosphor_amd_sink_work": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fosphor_amd_sink_ui_action": (None, [C.c_void_p, C.c_int]),
    "fosphor_amd_sink_reshape": (None, [C.c_void_p, C.c_int, C.c_int]),
    "fosphor_amd_sink_mouse_action": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "fosphor_amd_sink_set_freq_callback": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fosphor_amd_sink_write_prepare": (C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "fosphor_amd_sink_write_commit": (None, [C.c_void_p, C.c_int]),
    "fosphor_amd_sink_get_render": (None, [C.c_void_p, C.c_int, C.POINTER(Render)]),
    "fosphor_amd_sink_set_frequency_range": (None, [C.c_void_p, C.c_double, C.c_double]),
    "fosphor_amd_sink_set_fft_window": (None, [C.c_void_p, C.c_void_p]),
    "fosphor_amd_sink_set_visible": (None, [C.c_void_p, C.c_int]),
    "fosphor_amd_sink_core": (C.c_void_p, [C.c_void_p]),
    "fosphor_amd_sink_stats": (None, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fosphor_amd_process_device_overlap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fosphor_amd_set_overlap": (C.c_int, [C.c_void_p, C.c_int]),
    "fosphor_amd_traffic_twin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
}

_lib = None


def build(verbose=False):
    """hipcc --offload-arch=gfx950 build of the library (cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", ROOT, "all"], stdout=out)
    return LIB_PATH


def load():
    """Load the HIP library.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "gr-fosphor_amd: %s is missing -- run `make` (or __graft_entry__.build()); "
                "there is no CPU fallback" % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so (SONAME
        # libamdhip64.so.7, like /opt/rocm's) but libtorch_hip asks for it by the unversioned
        # file name, so if THIS library is loaded first (pulling in /opt/rocm's copy) a later
        # `import torch` loads a second runtime and device init fails.  Importing torch first
        # makes both bind to the one runtime, so pointers, streams and events are shared.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)		# AttributeError = the library does not export the header's symbol
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib
