"""Loader of librustradio_amd.so (the C ABI in include/rustradio_amd.h).

The library is the product; this module only binds it.  Import fails loudly when
the shared object is missing — there is no Python or CPU fallback for the hot path."""
from __future__ import annotations

import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# RR_LIB_PATH: measurement tools load a differently-built library (tools/*.sh: ablation / timing builds) without ever
# overwriting the product .so
LIB_PATH = os.environ.get("RR_LIB_PATH") or os.path.join(_HERE, "lib", "librustradio_amd.so")

# every symbol include/rustradio_amd.h declares (checked by tests/test_abi_symbols.py)
SYMBOLS = [
    "rr_abi_version", "rr_last_error", "rr_device_count", "rr_set_device", "rr_next_create_options",
    "rr_max_attenuation", "rr_make_window", "rr_compute_ntaps", "rr_low_pass", "rr_low_pass_complex",
    "rr_hilbert_taps", "rr_multiband",
    "rr_fir_c32_create", "rr_fir_f32_create", "rr_fftfilter_create", "rr_fftfilter_float_create",
    "rr_resampler_create", "rr_quaddemod_create", "rr_rtlsdr_decode_create", "rr_fftstream_create", "rr_fft_process", "rr_multiply_const_f32_create", "rr_multiply_const_c32_create", "rr_add_const_f32_create", "rr_add_const_c32_create", "rr_fastfm_create", "rr_hilbert_create", "rr_fm_chain_create", "rr_fm_chain_u8_create", "rr_fir_fftfilter_create", "rr_fir_fm_chain_create", "rr_audio_chain_create", "rr_vco_create", "rr_fm_tx_create", "rr_complex_to_mag2_create", "rr_airspy_decode_create", "rr_am_demod_create", "rr_am_demod_push_dev", "rr_am_demod_push", "rr_am_demod_dims", "rr_single_pole_iir_create", "rr_burst_detector_create", "rr_burst_edges", "rr_binary_slicer_create", "rr_nrzi_decode_create", "rr_descrambler_create", "rr_correlate_access_code_tag_create", "rr_bit_decoder_create", "rr_bit_tags", "rr_wpcr_create", "rr_wpcr_process_dev", "rr_wpcr_process", "rr_wpcr_results", "rr_debug_wpcr_spectrum", "rr_stream_to_pdu_create", "rr_stream_to_pdu_push_dev", "rr_stream_to_pdu_push", "rr_pdu_records", "rr_pdu_edges", "rr_pdu_arena_dev", "rr_pdu_fetch", "rr_debug_pdu_ranks", "rr_wpcr_process_pdus", "rr_stream_to_pdu_c32_create", "rr_stream_to_pdu_push_c32", "rr_pdu_fetch_c32", "rr_delay_create", "rr_burst_saver_create", "rr_burst_saver_push_dev", "rr_burst_saver_push", "rr_burst_saver_dims", "rr_wpcr_pack_dev", "rr_nrzi_encode_create", "rr_scrambler_g3ruh_create", "rr_hdlc_framer_create", "rr_hdlc_framer_bound", "rr_hdlc_framer_push_dev", "rr_hdlc_framer_push", "rr_hdlc_framer_records", "rr_hdlc_framer_dims", "rr_hdlc_framer_produced_dev", "rr_hdlc_deframer_create", "rr_hdlc_deframer_push_dev", "rr_hdlc_deframer_push", "rr_hdlc_frames", "rr_hdlc_frame_bytes", "rr_hdlc_bytes_dev", "rr_hdlc_stats", "rr_hdlc_deframer_dims", "rr_kiss_decode_create", "rr_kiss_decode_push_dev", "rr_kiss_decode_push", "rr_kiss_packets", "rr_kiss_packet_bytes", "rr_kiss_packet_bytes_dev", "rr_kiss_decode_stats", "rr_kiss_decode_dims", "rr_kiss_encode_create", "rr_kiss_encode_bound", "rr_kiss_encode_push_dev", "rr_kiss_encode_push", "rr_kiss_encode_records", "rr_kiss_encode_dims", "rr_kiss_encode_frames", "rr_hdlc_framer_push_kiss", "rr_symbol_sync_create", "rr_symbol_sync_push_dev", "rr_symbol_sync_push", "rr_symbol_sync_produced", "rr_symbol_sync_counts_dev", "rr_symbol_sync_dims", "rr_debug_symbol_sync_state", "rr_afsk_demod_create", "rr_afsk_demod_push_dev", "rr_afsk_demod_push", "rr_afsk_demod_dims", "rr_fsk_tx_create", "rr_fsk_tx_count", "rr_fsk_tx_push_dev", "rr_fsk_tx_push", "rr_fsk_tx_dims", "rr_fsk_tx_multi_create", "rr_fsk_tx_multi_bound", "rr_fsk_tx_multi_push_dev", "rr_fsk_tx_multi_push", "rr_fsk_tx_multi_counts", "rr_fsk_tx_multi_counts_dev", "rr_fsk_tx_multi_positions", "rr_fsk_tx_multi_dims", "rr_hdlc_receiver_create", "rr_hdlc_receiver_push_dev", "rr_hdlc_receiver_push", "rr_hdlc_receiver_frames", "rr_hdlc_receiver_frame_bytes", "rr_hdlc_receiver_bytes_dev", "rr_hdlc_receiver_stats", "rr_hdlc_receiver_consumed", "rr_hdlc_receiver_dims", "rr_il2p_receiver_create", "rr_il2p_receiver_push_dev", "rr_il2p_receiver_push", "rr_il2p_receiver_headers", "rr_il2p_receiver_stats", "rr_il2p_receiver_consumed", "rr_il2p_receiver_dims", "rr_pwm_decoder_create", "rr_pwm_decoder_push_dev", "rr_pwm_decoder_push", "rr_pwm_decoder_flush", "rr_pwm_frames", "rr_pwm_frame_bits", "rr_pwm_bits_dev", "rr_pwm_decoder_dims", "rr_hilbert_fir_create", "rr_fm_multi_create", "rr_fm_multi_u8_create", "rr_channelizer_create", "rr_channelizer_u8_create", "rr_fm_receiver_create", "rr_fm_receiver_u8_create", "rr_block_out_windows", "rr_block_destroy",
    "rr_block_work", "rr_block_work_dev", "rr_block_eof", "rr_block_name", "rr_block_tag_rule", "rr_block_in_elem_size",
    "rr_block_out_elem_size", "rr_block_sync", "rr_fftfilter_dims", "rr_fir_fft_tile", "rr_fir_set_rotator_mode",
    "rr_block_set_profiling", "rr_block_profile", "rr_debug_fft_stamps", "rr_debug_kernel_launches",
    "rr_debug_last_kernel",
    "rr_host_register", "rr_host_unregister", "rr_host_window_in_place",
    "rr_dstream_create", "rr_dstream_destroy", "rr_dstream_capacity", "rr_dstream_is_double_mapped", "rr_dstream_read_buf", "rr_dstream_write_buf",
    "rr_dstream_consume", "rr_dstream_produce", "rr_dstream_close", "rr_dstream_closed", "rr_dstream_wait", "rr_dstream_id", "rr_dstream_copy_in", "rr_dstream_copy_out", "rr_dstream_copy", "rr_block_work_streams",
    "rr_fanout_unique_id", "rr_fanout_create", "rr_fanout_destroy", "rr_fanout_produce_buf", "rr_fanout_submit",
    "rr_fanout_acquire", "rr_fanout_release", "rr_fanout_stats",
]

_lib = None


class BuildOpts(C.Structure):
    """rr_build_opts (include/rustradio_amd.h): path-selection overrides for the next create call"""
    _fields_ = [(n, C.c_int) for n in ("fir_path", "fir_prune", "fir_half", "fir_cfg_plus1", "fft_log2f", "fft_no_split",
                                        "fftfloat_complex", "fm_full", "fm_poly", "dstream_no_vmm", "fir_poly", "fft_nonfinite_tiles", "host_in_staged", "sync_lanes", "sync_prof_launch")] + [("reserved", C.c_int * 1)]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C rustradio_amd/csrc` (hipcc --offload-arch=gfx950). rustradio_amd has no CPU fallback.")
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64, and whichever copy is loaded
    # first serves both (same SONAME).  If this library pulled in /opt/rocm's copy before torch was imported,
    # torch would later run on a runtime it was not built against (observed: torch.cuda.is_available() False,
    # or "no usable HIP device" here).  So when torch is installed, let it load its runtime first.
    if "torch" not in sys.modules and not os.environ.get("RR_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    sz, f32, vp, i32 = C.c_size_t, C.c_float, C.c_void_p, C.c_int
    psz = C.POINTER(sz)
    L.rr_abi_version.restype = i32
    L.rr_last_error.restype = C.c_char_p
    L.rr_device_count.restype = i32
    L.rr_set_device.argtypes = [i32]; L.rr_set_device.restype = i32
    L.rr_next_create_options.argtypes = [vp]; L.rr_next_create_options.restype = i32
    L.rr_max_attenuation.argtypes = [i32]; L.rr_max_attenuation.restype = f32
    L.rr_make_window.argtypes = [i32, f32, sz, vp]; L.rr_make_window.restype = i32
    L.rr_compute_ntaps.argtypes = [f32, f32, i32]; L.rr_compute_ntaps.restype = sz
    L.rr_low_pass.argtypes = [f32, f32, f32, i32, f32, vp, sz]; L.rr_low_pass.restype = sz
    L.rr_low_pass_complex.argtypes = [f32, f32, f32, i32, f32, vp, sz]; L.rr_low_pass_complex.restype = sz
    L.rr_hilbert_taps.argtypes = [vp, sz, vp]; L.rr_hilbert_taps.restype = i32
    L.rr_multiband.argtypes = [vp, sz, vp, sz, vp]; L.rr_multiband.restype = i32
    L.rr_fir_c32_create.argtypes = [vp, sz, sz, i32, f32, f32]; L.rr_fir_c32_create.restype = vp
    L.rr_fir_f32_create.argtypes = [vp, sz, sz]; L.rr_fir_f32_create.restype = vp
    L.rr_fftfilter_create.argtypes = [vp, sz]; L.rr_fftfilter_create.restype = vp
    L.rr_fftfilter_float_create.argtypes = [vp, sz]; L.rr_fftfilter_float_create.restype = vp
    L.rr_resampler_create.argtypes = [sz, sz, sz]; L.rr_resampler_create.restype = vp
    L.rr_quaddemod_create.argtypes = [f32, i32]; L.rr_quaddemod_create.restype = vp
    L.rr_rtlsdr_decode_create.argtypes = []; L.rr_rtlsdr_decode_create.restype = vp
    L.rr_multiply_const_f32_create.argtypes = [f32]; L.rr_multiply_const_f32_create.restype = vp
    L.rr_multiply_const_c32_create.argtypes = [f32, f32]; L.rr_multiply_const_c32_create.restype = vp
    L.rr_add_const_f32_create.argtypes = [f32]; L.rr_add_const_f32_create.restype = vp
    L.rr_add_const_c32_create.argtypes = [f32, f32]; L.rr_add_const_c32_create.restype = vp
    L.rr_fastfm_create.argtypes = []; L.rr_fastfm_create.restype = vp
    L.rr_vco_create.argtypes = [C.c_ulonglong]; L.rr_vco_create.restype = vp
    L.rr_fm_tx_create.argtypes = [sz, sz, C.c_ulonglong]; L.rr_fm_tx_create.restype = vp
    L.rr_complex_to_mag2_create.argtypes = []; L.rr_complex_to_mag2_create.restype = vp
    L.rr_airspy_decode_create.argtypes = []; L.rr_airspy_decode_create.restype = vp
    L.rr_single_pole_iir_create.argtypes = [f32, sz]; L.rr_single_pole_iir_create.restype = vp
    L.rr_burst_detector_create.argtypes = [f32, f32]; L.rr_burst_detector_create.restype = vp
    L.rr_burst_edges.argtypes = [vp, vp, vp, sz, psz]; L.rr_burst_edges.restype = i32
    u64 = C.c_ulonglong
    L.rr_binary_slicer_create.argtypes = []; L.rr_binary_slicer_create.restype = vp
    L.rr_nrzi_decode_create.argtypes = []; L.rr_nrzi_decode_create.restype = vp
    L.rr_descrambler_create.argtypes = [u64, u64, C.c_uint]; L.rr_descrambler_create.restype = vp
    L.rr_correlate_access_code_tag_create.argtypes = [u64, C.c_uint, sz]; L.rr_correlate_access_code_tag_create.restype = vp
    L.rr_bit_decoder_create.argtypes = [i32, u64, u64, C.c_uint, u64, C.c_uint, sz]; L.rr_bit_decoder_create.restype = vp
    L.rr_bit_tags.argtypes = [vp, vp, vp, sz, psz]; L.rr_bit_tags.restype = i32
    L.rr_wpcr_create.argtypes = [f32]; L.rr_wpcr_create.restype = vp
    L.rr_wpcr_process_dev.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, vp]; L.rr_wpcr_process_dev.restype = i32
    L.rr_wpcr_process.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp]; L.rr_wpcr_process.restype = i32
    L.rr_wpcr_results.argtypes = [vp, vp, sz, psz]; L.rr_wpcr_results.restype = i32
    L.rr_debug_wpcr_spectrum.argtypes = [vp, sz, vp, sz, psz]; L.rr_debug_wpcr_spectrum.restype = i32
    L.rr_stream_to_pdu_create.argtypes = [f32, sz, sz, i32]; L.rr_stream_to_pdu_create.restype = vp
    L.rr_stream_to_pdu_push_dev.argtypes = [vp, vp, vp, sz, vp]; L.rr_stream_to_pdu_push_dev.restype = i32
    L.rr_stream_to_pdu_push.argtypes = [vp, vp, vp, sz]; L.rr_stream_to_pdu_push.restype = i32
    L.rr_pdu_records.argtypes = [vp, vp, sz, psz]; L.rr_pdu_records.restype = i32
    L.rr_pdu_edges.argtypes = [vp, vp, vp, sz, psz]; L.rr_pdu_edges.restype = i32
    L.rr_pdu_arena_dev.argtypes = [vp, psz]; L.rr_pdu_arena_dev.restype = vp
    L.rr_pdu_fetch.argtypes = [vp, sz, vp, sz]; L.rr_pdu_fetch.restype = i32
    L.rr_debug_pdu_ranks.argtypes = [vp, sz, vp, vp]; L.rr_debug_pdu_ranks.restype = i32
    L.rr_wpcr_process_pdus.argtypes = [vp, vp, vp, vp]; L.rr_wpcr_process_pdus.restype = i32
    L.rr_stream_to_pdu_c32_create.argtypes = [f32, sz, sz]; L.rr_stream_to_pdu_c32_create.restype = vp
    L.rr_stream_to_pdu_push_c32.argtypes = [vp, vp, vp, sz]; L.rr_stream_to_pdu_push_c32.restype = i32
    L.rr_pdu_fetch_c32.argtypes = [vp, sz, vp, sz]; L.rr_pdu_fetch_c32.restype = i32
    L.rr_delay_create.argtypes = [sz, sz]; L.rr_delay_create.restype = vp
    L.rr_burst_saver_create.argtypes = [f32, f32, sz, sz, sz]; L.rr_burst_saver_create.restype = vp
    L.rr_burst_saver_push_dev.argtypes = [vp, vp, sz, vp, vp]; L.rr_burst_saver_push_dev.restype = i32
    L.rr_burst_saver_push.argtypes = [vp, vp, sz, vp]; L.rr_burst_saver_push.restype = i32
    L.rr_burst_saver_dims.argtypes = [vp, sz, psz, psz]; L.rr_burst_saver_dims.restype = i32
    L.rr_wpcr_pack_dev.argtypes = [vp, vp, vp, sz, psz, vp, vp, sz, psz, vp]; L.rr_wpcr_pack_dev.restype = i32
    L.rr_nrzi_encode_create.argtypes = []; L.rr_nrzi_encode_create.restype = vp
    L.rr_scrambler_g3ruh_create.argtypes = []; L.rr_scrambler_g3ruh_create.restype = vp
    L.rr_hdlc_framer_create.argtypes = [i32, f32, f32]; L.rr_hdlc_framer_create.restype = vp
    L.rr_hdlc_framer_bound.argtypes = [vp, vp, sz]; L.rr_hdlc_framer_bound.restype = sz
    L.rr_hdlc_framer_push_dev.argtypes = [vp, vp, sz, vp, vp, sz, vp, sz, vp]; L.rr_hdlc_framer_push_dev.restype = i32
    L.rr_hdlc_framer_push.argtypes = [vp, vp, sz, vp, vp, sz, vp, sz, psz]; L.rr_hdlc_framer_push.restype = i32
    L.rr_hdlc_framer_records.argtypes = [vp, vp, sz, psz, psz]; L.rr_hdlc_framer_records.restype = i32
    L.rr_hdlc_framer_dims.argtypes = [vp, psz]; L.rr_hdlc_framer_dims.restype = i32
    L.rr_hdlc_framer_produced_dev.argtypes = [vp]; L.rr_hdlc_framer_produced_dev.restype = vp
    pu64 = C.POINTER(C.c_ulonglong)
    L.rr_hdlc_deframer_create.argtypes = [sz, sz, i32]; L.rr_hdlc_deframer_create.restype = vp
    L.rr_hdlc_deframer_push_dev.argtypes = [vp, vp, sz, vp]; L.rr_hdlc_deframer_push_dev.restype = i32
    L.rr_hdlc_deframer_push.argtypes = [vp, vp, sz]; L.rr_hdlc_deframer_push.restype = i32
    L.rr_hdlc_frames.argtypes = [vp, vp, sz, psz]; L.rr_hdlc_frames.restype = i32
    L.rr_hdlc_frame_bytes.argtypes = [vp, vp, sz, psz]; L.rr_hdlc_frame_bytes.restype = i32
    L.rr_hdlc_bytes_dev.argtypes = [vp, psz]; L.rr_hdlc_bytes_dev.restype = vp
    L.rr_hdlc_stats.argtypes = [vp, pu64, pu64, pu64]; L.rr_hdlc_stats.restype = i32
    L.rr_hdlc_deframer_dims.argtypes = [vp, psz, psz]; L.rr_hdlc_deframer_dims.restype = i32
    # rr_kiss_decode / rr_kiss_encode
    L.rr_kiss_decode_create.argtypes = [sz]; L.rr_kiss_decode_create.restype = vp
    L.rr_kiss_decode_push_dev.argtypes = [vp, vp, sz, vp]; L.rr_kiss_decode_push_dev.restype = i32
    L.rr_kiss_decode_push.argtypes = [vp, vp, sz]; L.rr_kiss_decode_push.restype = i32
    L.rr_kiss_packets.argtypes = [vp, vp, sz, psz]; L.rr_kiss_packets.restype = i32
    L.rr_kiss_packet_bytes.argtypes = [vp, vp, sz, psz]; L.rr_kiss_packet_bytes.restype = i32
    L.rr_kiss_packet_bytes_dev.argtypes = [vp, psz]; L.rr_kiss_packet_bytes_dev.restype = vp
    L.rr_kiss_decode_stats.argtypes = [vp, pu64]; L.rr_kiss_decode_stats.restype = i32
    L.rr_kiss_decode_dims.argtypes = [vp, psz, psz, psz]; L.rr_kiss_decode_dims.restype = i32
    L.rr_kiss_encode_create.argtypes = []; L.rr_kiss_encode_create.restype = vp
    L.rr_kiss_encode_bound.argtypes = [vp, sz]; L.rr_kiss_encode_bound.restype = sz
    L.rr_kiss_encode_push_dev.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, sz, vp]; L.rr_kiss_encode_push_dev.restype = i32
    L.rr_kiss_encode_push.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, sz, psz]; L.rr_kiss_encode_push.restype = i32
    L.rr_kiss_encode_records.argtypes = [vp, vp, sz, psz, psz]; L.rr_kiss_encode_records.restype = i32
    L.rr_kiss_encode_dims.argtypes = [vp, psz, psz]; L.rr_kiss_encode_dims.restype = i32
    L.rr_kiss_encode_frames.argtypes = [vp, vp, vp, sz, vp, sz, vp]; L.rr_kiss_encode_frames.restype = i32
    L.rr_hdlc_framer_push_kiss.argtypes = [vp, vp, vp, sz, vp]; L.rr_hdlc_framer_push_kiss.restype = i32
    # rr_pwm_decoder
    L.rr_pwm_decoder_create.argtypes = [f32, f32, sz, sz, sz, sz, sz, sz, sz, sz, sz, i32, sz]; L.rr_pwm_decoder_create.restype = vp
    L.rr_pwm_decoder_push_dev.argtypes = [vp, vp, sz, vp]; L.rr_pwm_decoder_push_dev.restype = i32
    L.rr_pwm_decoder_push.argtypes = [vp, vp, sz]; L.rr_pwm_decoder_push.restype = i32
    L.rr_pwm_decoder_flush.argtypes = [vp, vp]; L.rr_pwm_decoder_flush.restype = i32
    L.rr_pwm_frames.argtypes = [vp, vp, sz, psz]; L.rr_pwm_frames.restype = i32
    L.rr_pwm_frame_bits.argtypes = [vp, vp, sz, psz]; L.rr_pwm_frame_bits.restype = i32
    L.rr_pwm_bits_dev.argtypes = [vp, psz]; L.rr_pwm_bits_dev.restype = vp
    L.rr_pwm_decoder_dims.argtypes = [vp, psz]; L.rr_pwm_decoder_dims.restype = i32
    L.rr_symbol_sync_create.argtypes = [f32, f32, vp, sz, sz]; L.rr_symbol_sync_create.restype = vp
    L.rr_symbol_sync_push_dev.argtypes = [vp, vp, sz, sz, vp, vp, sz, vp]; L.rr_symbol_sync_push_dev.restype = i32
    L.rr_symbol_sync_push.argtypes = [vp, vp, sz, sz, vp, vp, sz, psz]; L.rr_symbol_sync_push.restype = i32
    L.rr_symbol_sync_produced.argtypes = [vp, psz, sz, psz]; L.rr_symbol_sync_produced.restype = i32
    L.rr_symbol_sync_counts_dev.argtypes = [vp]; L.rr_symbol_sync_counts_dev.restype = vp
    L.rr_symbol_sync_dims.argtypes = [vp, psz]; L.rr_symbol_sync_dims.restype = i32
    L.rr_debug_symbol_sync_state.argtypes = [vp, sz, vp, C.POINTER(i32), vp, sz, psz]; L.rr_debug_symbol_sync_state.restype = i32
    L.rr_hdlc_receiver_create.argtypes = [sz, i32, u64, u64, C.c_uint, sz, sz, i32]; L.rr_hdlc_receiver_create.restype = vp
    L.rr_hdlc_receiver_push_dev.argtypes = [vp, vp, sz, sz, vp, vp]; L.rr_hdlc_receiver_push_dev.restype = i32
    L.rr_hdlc_receiver_push.argtypes = [vp, vp, sz, sz, psz]; L.rr_hdlc_receiver_push.restype = i32
    L.rr_hdlc_receiver_frames.argtypes = [vp, vp, sz, psz]; L.rr_hdlc_receiver_frames.restype = i32
    L.rr_hdlc_receiver_frame_bytes.argtypes = [vp, vp, sz, psz]; L.rr_hdlc_receiver_frame_bytes.restype = i32
    L.rr_hdlc_receiver_bytes_dev.argtypes = [vp, psz]; L.rr_hdlc_receiver_bytes_dev.restype = vp
    L.rr_hdlc_receiver_stats.argtypes = [vp, vp, vp, vp, sz, psz]; L.rr_hdlc_receiver_stats.restype = i32
    L.rr_hdlc_receiver_consumed.argtypes = [vp, vp, sz, psz]; L.rr_hdlc_receiver_consumed.restype = i32
    L.rr_hdlc_receiver_dims.argtypes = [vp, psz, psz]; L.rr_hdlc_receiver_dims.restype = i32
    L.rr_il2p_receiver_create.argtypes = [sz, i32, sz]; L.rr_il2p_receiver_create.restype = vp
    L.rr_il2p_receiver_push_dev.argtypes = [vp, vp, sz, sz, vp, vp]; L.rr_il2p_receiver_push_dev.restype = i32
    L.rr_il2p_receiver_push.argtypes = [vp, vp, sz, sz, psz]; L.rr_il2p_receiver_push.restype = i32
    L.rr_il2p_receiver_headers.argtypes = [vp, vp, sz, psz]; L.rr_il2p_receiver_headers.restype = i32
    L.rr_il2p_receiver_stats.argtypes = [vp, vp, vp, sz, psz]; L.rr_il2p_receiver_stats.restype = i32
    L.rr_il2p_receiver_consumed.argtypes = [vp, vp, sz, psz]; L.rr_il2p_receiver_consumed.restype = i32
    L.rr_il2p_receiver_dims.argtypes = [vp, psz, psz]; L.rr_il2p_receiver_dims.restype = i32
    L.rr_afsk_demod_create.argtypes = [sz, sz, i32, f32, f32, vp, sz, f32]; L.rr_afsk_demod_create.restype = vp
    L.rr_afsk_demod_push_dev.argtypes = [vp, vp, sz, sz, vp, sz, psz, vp]; L.rr_afsk_demod_push_dev.restype = i32
    L.rr_afsk_demod_push.argtypes = [vp, vp, sz, sz, vp, sz, psz]; L.rr_afsk_demod_push.restype = i32
    L.rr_afsk_demod_dims.argtypes = [vp, psz, psz]; L.rr_afsk_demod_dims.restype = i32
    L.rr_am_demod_create.argtypes = [sz, vp, sz, sz, sz, f32]; L.rr_am_demod_create.restype = vp
    L.rr_am_demod_push_dev.argtypes = [vp, vp, sz, sz, vp, sz, psz, vp]; L.rr_am_demod_push_dev.restype = i32
    L.rr_am_demod_push.argtypes = [vp, vp, sz, sz, vp, sz, psz]; L.rr_am_demod_push.restype = i32
    L.rr_am_demod_dims.argtypes = [vp, psz, psz]; L.rr_am_demod_dims.restype = i32
    L.rr_fsk_tx_create.argtypes = [i32, sz, sz, f32, f32, u64, f32, sz, sz, u64]; L.rr_fsk_tx_create.restype = vp
    L.rr_fsk_tx_count.argtypes = [vp, sz, psz, psz]; L.rr_fsk_tx_count.restype = i32
    L.rr_fsk_tx_push_dev.argtypes = [vp, vp, sz, vp, sz, vp, sz, psz, psz, vp]; L.rr_fsk_tx_push_dev.restype = i32
    L.rr_fsk_tx_push.argtypes = [vp, vp, sz, vp, sz, vp, sz, psz, psz]; L.rr_fsk_tx_push.restype = i32
    L.rr_fsk_tx_dims.argtypes = [vp, psz, psz, psz]; L.rr_fsk_tx_dims.restype = i32
    L.rr_fsk_tx_multi_create.argtypes = [sz, i32, sz, sz, f32, f32, u64, f32, sz, sz, u64]; L.rr_fsk_tx_multi_create.restype = vp
    L.rr_fsk_tx_multi_bound.argtypes = [vp, sz, psz, psz]; L.rr_fsk_tx_multi_bound.restype = i32
    L.rr_fsk_tx_multi_push_dev.argtypes = [vp, vp, sz, sz, vp, vp, sz, vp, sz, vp]; L.rr_fsk_tx_multi_push_dev.restype = i32
    L.rr_fsk_tx_multi_push.argtypes = [vp, vp, sz, sz, psz, vp, sz, vp, sz, psz, psz]; L.rr_fsk_tx_multi_push.restype = i32
    L.rr_fsk_tx_multi_counts.argtypes = [vp, vp, vp, sz, psz]; L.rr_fsk_tx_multi_counts.restype = i32
    L.rr_fsk_tx_multi_counts_dev.argtypes = [vp]; L.rr_fsk_tx_multi_counts_dev.restype = vp
    L.rr_fsk_tx_multi_positions.argtypes = [vp, vp, vp, vp, sz, psz]; L.rr_fsk_tx_multi_positions.restype = i32
    L.rr_fsk_tx_multi_dims.argtypes = [vp, psz, psz, psz]; L.rr_fsk_tx_multi_dims.restype = i32
    L.rr_fftstream_create.argtypes = [sz]; L.rr_fftstream_create.restype = vp
    L.rr_fft_process.argtypes = [vp, vp, sz, vp]; L.rr_fft_process.restype = i32
    L.rr_hilbert_create.argtypes = [sz, i32, f32]; L.rr_hilbert_create.restype = vp
    L.rr_fm_chain_create.argtypes = [vp, sz, sz, sz, f32, i32]; L.rr_fm_chain_create.restype = vp
    L.rr_fir_fftfilter_create.argtypes = [vp, sz, vp, sz]; L.rr_fir_fftfilter_create.restype = vp
    L.rr_fir_fm_chain_create.argtypes = [vp, sz, vp, sz, sz, sz, f32, i32]; L.rr_fir_fm_chain_create.restype = vp
    L.rr_audio_chain_create.argtypes = [vp, sz, sz, sz, f32]; L.rr_audio_chain_create.restype = vp
    L.rr_fm_chain_u8_create.argtypes = [vp, sz, sz, sz, f32, i32]; L.rr_fm_chain_u8_create.restype = vp
    L.rr_hilbert_fir_create.argtypes = [sz, i32, f32, vp, sz, sz, i32, f32, f32]; L.rr_hilbert_fir_create.restype = vp
    L.rr_fm_multi_create.argtypes = [vp, sz, sz, sz, sz, f32, i32]; L.rr_fm_multi_create.restype = vp
    L.rr_fm_multi_u8_create.argtypes = [vp, sz, sz, sz, sz, f32, i32]; L.rr_fm_multi_u8_create.restype = vp
    L.rr_channelizer_create.argtypes = [vp, sz, sz, sz, sz]; L.rr_channelizer_create.restype = vp
    L.rr_channelizer_u8_create.argtypes = [vp, sz, sz, sz, sz]; L.rr_channelizer_u8_create.restype = vp
    L.rr_fm_receiver_create.argtypes = [vp, sz, sz, sz, sz, f32, i32, vp, sz, sz, sz, f32]; L.rr_fm_receiver_create.restype = vp
    L.rr_fm_receiver_u8_create.argtypes = [vp, sz, sz, sz, sz, f32, i32, vp, sz, sz, sz, f32]; L.rr_fm_receiver_u8_create.restype = vp
    L.rr_block_out_windows.argtypes = [vp]; L.rr_block_out_windows.restype = sz
    L.rr_block_destroy.argtypes = [vp]; L.rr_block_destroy.restype = None
    L.rr_block_work.argtypes = [vp, vp, sz, vp, sz, psz, psz, psz]; L.rr_block_work.restype = i32
    L.rr_block_work_dev.argtypes = [vp, vp, sz, vp, sz, psz, psz, psz, vp]; L.rr_block_work_dev.restype = i32
    L.rr_block_eof.argtypes = [vp, i32]; L.rr_block_eof.restype = i32
    L.rr_block_name.argtypes = [vp]; L.rr_block_name.restype = C.c_char_p
    L.rr_block_tag_rule.argtypes = [vp, psz]; L.rr_block_tag_rule.restype = i32
    L.rr_block_in_elem_size.argtypes = [vp]; L.rr_block_in_elem_size.restype = sz
    L.rr_block_out_elem_size.argtypes = [vp]; L.rr_block_out_elem_size.restype = sz
    L.rr_block_sync.argtypes = [vp]; L.rr_block_sync.restype = i32
    L.rr_fftfilter_dims.argtypes = [vp, psz, psz, psz]; L.rr_fftfilter_dims.restype = i32
    L.rr_fir_fft_tile.argtypes = [vp]; L.rr_fir_fft_tile.restype = sz
    L.rr_fir_set_rotator_mode.argtypes = [vp, i32]; L.rr_fir_set_rotator_mode.restype = i32
    L.rr_debug_fft_stamps.argtypes = [vp]; L.rr_debug_fft_stamps.restype = i32
    L.rr_debug_kernel_launches.argtypes = []; L.rr_debug_kernel_launches.restype = C.c_ulonglong
    L.rr_debug_last_kernel.argtypes = [vp]; L.rr_debug_last_kernel.restype = C.c_char_p
    pvp = C.POINTER(vp)
    L.rr_host_register.argtypes = [vp, sz]; L.rr_host_register.restype = i32
    L.rr_host_window_in_place.argtypes = [vp, sz]; L.rr_host_window_in_place.restype = i32
    L.rr_host_unregister.argtypes = [vp]; L.rr_host_unregister.restype = i32
    L.rr_dstream_create.argtypes = [sz, sz]; L.rr_dstream_create.restype = vp
    L.rr_dstream_destroy.argtypes = [vp]; L.rr_dstream_destroy.restype = None
    L.rr_dstream_capacity.argtypes = [vp]; L.rr_dstream_capacity.restype = sz
    L.rr_dstream_is_double_mapped.argtypes = [vp]; L.rr_dstream_is_double_mapped.restype = i32
    L.rr_dstream_read_buf.argtypes = [vp, pvp]; L.rr_dstream_read_buf.restype = sz
    L.rr_dstream_write_buf.argtypes = [vp, pvp, vp]; L.rr_dstream_write_buf.restype = sz
    L.rr_dstream_consume.argtypes = [vp, sz]; L.rr_dstream_consume.restype = i32
    L.rr_dstream_produce.argtypes = [vp, sz]; L.rr_dstream_produce.restype = i32
    L.rr_dstream_close.argtypes = [vp, i32]; L.rr_dstream_close.restype = i32
    L.rr_dstream_closed.argtypes = [vp, i32]; L.rr_dstream_closed.restype = i32
    L.rr_dstream_wait.argtypes = [vp, i32, sz, C.c_uint, C.POINTER(C.c_int)]; L.rr_dstream_wait.restype = sz
    L.rr_dstream_id.argtypes = [vp]; L.rr_dstream_id.restype = sz
    L.rr_dstream_copy_in.argtypes = [vp, sz, vp, sz, vp]; L.rr_dstream_copy_in.restype = i32
    L.rr_dstream_copy_out.argtypes = [vp, sz, vp, sz, vp]; L.rr_dstream_copy_out.restype = i32
    L.rr_dstream_copy.argtypes = [vp, sz, vp, sz, sz, vp]; L.rr_dstream_copy.restype = i32
    L.rr_block_work_streams.argtypes = [vp, vp, vp, psz, psz, psz, vp]; L.rr_block_work_streams.restype = i32
    u64 = C.c_ulonglong
    L.rr_fanout_unique_id.argtypes = [vp]; L.rr_fanout_unique_id.restype = i32
    L.rr_fanout_create.argtypes = [vp, i32, i32, i32, sz, i32]; L.rr_fanout_create.restype = vp
    L.rr_fanout_destroy.argtypes = [vp]; L.rr_fanout_destroy.restype = None
    L.rr_fanout_produce_buf.argtypes = [vp, u64, vp]; L.rr_fanout_produce_buf.restype = vp
    L.rr_fanout_submit.argtypes = [vp, u64, vp]; L.rr_fanout_submit.restype = i32
    L.rr_fanout_acquire.argtypes = [vp, u64, vp]; L.rr_fanout_acquire.restype = vp
    L.rr_fanout_release.argtypes = [vp, u64, vp]; L.rr_fanout_release.restype = i32
    L.rr_fanout_stats.argtypes = [vp, C.POINTER(C.c_double), psz]; L.rr_fanout_stats.restype = i32
    L.rr_block_set_profiling.argtypes = [vp, i32]; L.rr_block_set_profiling.restype = i32
    L.rr_block_profile.argtypes = [vp, C.POINTER(C.c_double), psz, i32]; L.rr_block_profile.restype = i32
    _lib = L
    return L


def last_error() -> str:
    return lib().rr_last_error().decode()
