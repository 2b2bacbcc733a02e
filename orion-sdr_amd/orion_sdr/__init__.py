"""orion_sdr (MI355X engine) — Python mirror of skynavga/orion-sdr's analog API.

Same class names, constructor arguments and ``process(ndarray) -> ndarray``
contract as the reference PyO3 module (``python/orion_sdr/__init__.pyi:18-79``,
``src/python/demodulate.rs:9-148``): IQ arrays are ``numpy.complex64``, audio
``numpy.float32``, inputs must be 1-D and C-contiguous (else ``ValueError`` /
``TypeError``), every call returns a new array, and instances keep their
streaming state between calls.

Every class runs on the GPU through ``lib/liborion_sdr_amd.so`` (gfx950 HIP
kernels behind the C ABI in ``include/orion_sdr_amd.h``). There is no CPU
fallback: importing without the built library, or calling without a visible
device, raises.

``process`` also accepts torch CUDA tensors (device path, no host copies): the
output is a new torch tensor on the same device, computed asynchronously on
torch's current stream.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

__all__ = [
    "Rotator", "Nco", "Biquad", "LpDcCascade", "PmDirectPhaseMod", "CwKeyedMod", "TxLowpass", "FirDecimator", "FirLowpass", "FirLowpassIq", "LpCascade", "DcBlocker",
    "FmQuadratureDemod", "PmQuadratureDemod", "SsbProductDemod", "AmEnvelopeDemod",
    "CwEnvelopeDemod", "WbfmChain", "AgcRms", "AgcRmsIq", "AmDsbMod", "FmPhaseAccumMod", "SsbPhasingMod",
    "fir_lowpass_design", "kaiser_lowpass_taps",
    "kaiser_transition_norm", "kaiser_num_taps", "lp_cascade_design", "lib_path", "OrionError", "diag_stream_read",
    "AudioToIqChain", "IqToIqChain", "IqToAudioChain", "Graph", "stream_shard", "STREAM_HALO",
    "SyncEngine", "CANDIDATE_DTYPE", "compute_waterfall", "find_candidates", "ft8_sync", "ft4_sync",
    "ft8_sync_batch", "ft4_sync_batch", "sync_geometry",
    "Ft8Codec", "Ft4Codec", "RESULT_DTYPE", "PICK_DTYPE", "LDPC_N", "ldpc_decode_batch", "ldpc_decode_host",
    "ldpc_tables", "ft_crc14", "ft8_decode", "ft4_decode", "ft8_decode_batch", "ft4_decode_batch",
    "Ft8Mod", "Ft4Mod", "Ft8Demod", "Ft4Demod", "ft8_synth", "ft4_synth", "SIGNAL_DTYPE", "FT8_FRAME_LEN",
    "FT4_FRAME_LEN",
    "VaricodeEncoder", "VaricodeDecoder", "StreamingViterbi", "varicode_encode", "varicode_decode", "psk31_tables",
    "conv_encode", "viterbi_decode", "viterbi_decode_hard", "psk31_viterbi_batch", "VARICODE_MAX_BITS",
    "PSK31_TRACEBACK_DEPTH", "psk31_sps", "psk31_text_bits", "Bpsk31Mod", "Qpsk31Mod", "Bpsk31Demod", "Qpsk31Demod",
    "Bpsk31Decider", "Psk31DemodBank", "PSK31_STREAM_DTYPE", "PSK31_REPORT_DTYPE", "psk31_find_carriers", "psk31_find_carriers_device", "psk31_synth", "PSK31_SIGNAL_DTYPE", "psk31_rotator_q64",
    "psk31_sync", "psk31_sync_batch", "best_psk31_sync", "psk31_decode", "psk31_decode_batch", "Psk31Stream",
    "OfdmConfig", "OfdmMod", "OfdmDemod", "OfdmDecider", "OfdmSoftDemod", "OfdmEqualizer", "OfdmRxFrame",
    "build_ofdm_rx_frame", "FftBlock", "IfftBlock", "ofdm_modulate_batch", "ofdm_demodulate_batch", "ofdm_tables",
    "ofdm_map", "ofdm_decide", "ofdm_llr", "fft_host", "ofdm_window", "ofdm_rotator", "ofdm_equalizer_weight",
    "ofdm_interpolate", "ofdm_max_pilot_safe_backoff", "OFDM_CONSTELLATIONS", "OFDM_PLAN_ERRORS",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
# ORION_SDR_LIB: an alternative build of the same library (timing experiments)
_LIB = os.environ.get("ORION_SDR_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "liborion_sdr_amd.so")


def lib_path() -> str:
    return _LIB


class OrionError(RuntimeError):
    """A failure reported by the C ABI (HIP error, bad argument, ...)."""


class WorkReport(C.Structure):
    _fields_ = [("in_read", C.c_size_t), ("out_written", C.c_size_t)]


class TxLowpassSpec(C.Structure):
    _fields_ = [("cutoff_norm", C.c_float), ("num_taps", C.c_size_t), ("stopband_db", C.c_float)]


class WbfmParams(C.Structure):
    _fields_ = [("fs", C.c_float), ("f_off", C.c_float), ("dec_cutoff", C.c_float),
                ("dec_trans", C.c_float), ("dev_hz", C.c_float), ("audio_bw", C.c_float),
                ("audio_pass", C.c_float), ("audio_trans", C.c_float), ("m", C.c_size_t)]


def _load():
    if not os.path.exists(_LIB):
        raise ImportError(
            f"orion_sdr: native library {_LIB} is missing — build it with "
            "`make -C orion-sdr_amd` (hipcc, gfx950). There is no CPU fallback.")
    # The library and torch both need libamdhip64.so.7 (one soname: the first one
    # loaded serves the process). Load torch's first, as bench.py does, so torch's
    # own device path keeps the runtime it was built against whatever the import order.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_LIB)
    vp, sz, f, i = C.c_void_p, C.c_size_t, C.c_float, C.c_int
    fp = C.POINTER(C.c_float)
    sig = {
        "orion_version": (C.c_char_p, []), "orion_last_error": (C.c_char_p, []),
        "orion_device_count": (i, []), "orion_set_device": (i, [i]), "orion_synchronize": (i, [vp]),
        "orion_rotator_new": (vp, [f, f]),
        "orion_rotator_set_freq": (i, [vp, f, f]), "orion_rotator_reset_phase": (i, [vp]),
        "orion_rotator_mix_usb_block": (i, [vp, vp, sz, vp, sz, C.POINTER(WorkReport)]),
        "orion_rotator_mix_usb_block_device": (i, [vp, vp, sz, vp, sz, vp, C.POINTER(WorkReport)]),
        "orion_nco_new": (vp, [f, f]), "orion_nco_set_freq": (i, [vp, f]),
        "orion_nco_next_cs_block": (i, [vp, vp, sz]), "orion_nco_next_cs_block_device": (i, [vp, vp, sz, vp]),
        "orion_rotator_next_cs_block": (i, [vp, vp, sz]),
        "orion_rotator_next_cs_block_device": (i, [vp, vp, sz, vp]),
        "orion_osc_table_phasors": (i, [f, f, C.c_uint64, vp, sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64)]),
        "orion_fir_lowpass_iq_num_taps": (i, [vp, C.POINTER(sz)]),
        "orion_fir_lowpass_iq_group_delay": (i, [vp, C.POINTER(sz)]),
        "orion_biquad_new": (vp, [f, f, f, f, f]),
        "orion_lp_dc_cascade_new": (vp, [f, f, f]), "orion_lp_dc_cascade_set_sqrt_map": (i, [vp, i]),
        "orion_lp_dc_cascade_set_map": (i, [vp, i]),
        "orion_pm_direct_phase_mod_new": (vp, [f, f, f]), "orion_pm_direct_phase_mod_set_gain": (i, [vp, f]),
        "orion_pm_direct_phase_mod_set_sensitivity": (i, [vp, f]),
        "orion_cw_keyed_mod_new": (vp, [f, f, f, f]), "orion_cw_keyed_mod_set_gain": (i, [vp, f]),
        "orion_tx_lowpass_for_null_band": (TxLowpassSpec, [sz, sz, sz, f]),
        "orion_tx_lowpass_taps_for_null_band": (sz, [sz, sz, f]),
        "orion_tx_lowpass_group_delay": (sz, [C.POINTER(TxLowpassSpec)]),
        "orion_tx_lowpass_transition_norm": (f, [C.POINTER(TxLowpassSpec)]),
        "orion_tx_lowpass_transition_fits": (i, [C.POINTER(TxLowpassSpec), sz, sz]),
        "orion_tx_lowpass_stopband_edge_norm": (f, [C.POINTER(TxLowpassSpec)]),
        "orion_tx_lowpass_fits_guard": (i, [C.POINTER(TxLowpassSpec), sz, sz, sz]),
        "orion_tx_lowpass_filter": (vp, [C.POINTER(TxLowpassSpec)]),
        "orion_fir_decimator_new": (vp, [f, sz, f, f]),
        "orion_fir_decimator_batch_new": (vp, [f, sz, f, f, sz]),
        "orion_fir_lowpass_new": (vp, [f, f, f]),
        "orion_fir_lowpass_iq_design": (vp, [sz, f, f]),
        "orion_fir_lowpass_iq_from_taps": (vp, [fp, sz]),
        "orion_fir_lowpass_iq_batch_from_taps": (vp, [fp, sz, sz]),
        "orion_fir_lowpass_iq_filter_aligned_device": (i, [vp, vp, sz, vp]),
        "orion_fir_lowpass_iq_filter_aligned": (i, [vp, vp, sz]),
        "orion_lp_cascade_new": (vp, [f, f]),
        "orion_dc_blocker_new": (vp, [f, f]),
        "orion_fm_quadrature_demod_new": (vp, [f, f, f]),
        "orion_fm_quadrature_demod_with_translate": (i, [vp, f]),
        "orion_pm_quadrature_demod_new": (vp, [f, f, f]),
        "orion_ssb_product_demod_new": (vp, [f, f, f]),
        "orion_ssb_product_demod_batch_new": (vp, [f, f, f, sz]),
        "orion_am_envelope_demod_new": (vp, [f, f]),
        "orion_am_envelope_demod_with_abs_approx": (i, [vp, f, f]),
        "orion_cw_envelope_demod_new": (vp, [f, f, f]),
        "orion_cw_envelope_demod_set_gain": (i, [vp, f]),
        "orion_am_dsb_mod_new": (vp, [f, f, f, f]),
        "orion_agc_rms_new": (vp, [f, f, f, f]),
        "orion_agc_rms_iq_new": (vp, [f, f, f, f]),
        "orion_am_dsb_mod_set_gain": (i, [vp, f]),
        "orion_am_dsb_mod_set_clamp": (i, [vp, i]),
        "orion_fm_phase_accum_mod_new": (vp, [f, f, f]),
        "orion_fm_phase_accum_mod_set_deviation": (i, [vp, f]),
        "orion_fm_phase_accum_mod_set_gain": (i, [vp, f]),
        "orion_ssb_phasing_mod_new": (vp, [f, f, f, f, i]),
        "orion_wbfm_chain_new": (vp, [C.POINTER(WbfmParams)]),
        "orion_wbfm_chain_batch_new": (vp, [C.POINTER(WbfmParams), fp, sz]),
        "orion_wbfm_chain_configure": (i, [vp, i, i]),
        "orion_wbfm_chain_seek": (i, [vp, C.c_uint64]),
        "orion_block_process": (i, [vp, vp, sz, vp, sz, C.POINTER(WorkReport)]),
        "orion_block_process_device": (i, [vp, vp, sz, vp, sz, vp, C.POINTER(WorkReport)]),
        "orion_batch_process": (i, [vp, vp, sz, sz, vp, sz, vp, C.POINTER(WorkReport)]),
        "orion_block_reset": (i, [vp]), "orion_block_free": (None, [vp]),
        "orion_block_configure": (i, [vp, i, C.c_longlong]),
        "orion_block_status": (i, [vp]),
        "orion_debug_set_spin_limit": (None, [C.c_uint32]), "orion_debug_spin_limit": (C.c_uint32, []),
        "orion_block_in_type": (i, [vp]), "orion_block_out_type": (i, [vp]),
        "orion_block_out_len": (sz, [vp, sz]), "orion_block_channels": (sz, [vp]),
        "orion_block_name": (C.c_char_p, [vp]),
        "orion_block_taps": (i, [vp, i, fp, sz, C.POINTER(sz)]),
        "orion_fir_lowpass_design": (sz, [f, f, f, fp, sz]),
        "orion_kaiser_lowpass_taps": (sz, [sz, f, f, fp, sz]),
        "orion_kaiser_transition_norm": (f, [sz, f]),
        "orion_kaiser_num_taps": (sz, [f, f]),
        "orion_lp_cascade_design": (None, [f, f, fp]),
        "orion_diag_stream_read_bytes": (sz, [sz]),
        "orion_diag_stream_read": (i, [vp, sz, vp]),
        "orion_diag_spin": (i, [vp, C.c_uint32, C.c_uint32, C.c_double]),
        "orion_diag_stream_create": (vp, [C.c_uint32]), "orion_diag_stream_destroy": (i, [vp]),
        "orion_device_cus": (i, []),
        "orion_host_alloc": (vp, [sz]), "orion_host_free": (i, [vp]),
        "orion_sync_new": (vp, []), "orion_sync_free": (None, [vp]), "orion_sync_set_rows_per_lane": (i, [vp, i]),
        "orion_waterfall_compute": (i, [vp, vp, f, f, f, sz, sz, sz, sz, sz, sz, i, vp]),
        "orion_waterfall_compute_device": (i, [vp, vp, f, f, f, sz, sz, sz, sz, sz, sz, i, vp, vp]),
        "orion_costas_find_candidates_device": (i, [vp, vp, sz, sz, sz, i, i, i, sz, vp, vp, vp]),
        "orion_sync_llr_device": (i, [vp, sz, sz, sz, i, vp, vp, sz, vp, vp]),
        "orion_ft8_sync": (i, [vp, vp, sz, sz, f, f, f, i, i, sz, vp, vp, vp]),
        "orion_ft4_sync": (i, [vp, vp, sz, sz, f, f, f, i, i, sz, vp, vp, vp]),
        "orion_ft8_sync_device": (i, [vp, vp, sz, sz, f, f, f, i, i, sz, vp, vp, vp, vp]),
        "orion_ft4_sync_device": (i, [vp, vp, sz, sz, f, f, f, i, i, sz, vp, vp, vp, vp]),
        "orion_sync_geometry": (i, [i, f, f, i, i, C.POINTER(sz)]),
        "orion_ldpc_decode": (i, [vp, sz, vp, sz, i, i, sz, vp, vp]),
        "orion_ldpc_decode_device": (i, [vp, sz, vp, sz, i, i, sz, vp, vp, vp]),
        "orion_ft8_decode": (i, [vp, vp, sz, sz, f, f, f, i, i, sz, i, sz, vp, vp, vp, vp, vp]),
        "orion_ft4_decode": (i, [vp, vp, sz, sz, f, f, f, i, i, sz, i, sz, vp, vp, vp, vp, vp]),
        "orion_ft8_decode_device": (i, [vp, vp, sz, sz, f, f, f, i, i, sz, i, sz, vp, vp, vp, vp, vp, vp]),
        "orion_ft4_decode_device": (i, [vp, vp, sz, sz, f, f, f, i, i, sz, i, sz, vp, vp, vp, vp, vp, vp]),
        "orion_ft8_encode": (i, [vp, vp, vp]), "orion_ft4_encode": (i, [vp, vp, vp]),
        "orion_ft_frame_to_llr_hard": (i, [i, vp, vp]),
        "orion_ldpc_decode_host": (i, [vp, i, i, sz, vp, vp]),
        "orion_ft_crc14": (C.c_uint16, [vp, sz]),
        "orion_ldpc_tables": (i, [vp, vp, vp, vp]),
        "orion_ft_mod_new": (vp, [i, f, f, f, f]), "orion_ft_mod_free": (None, [vp]),
        "orion_ft_mod_modulate": (i, [vp, vp, sz, vp]), "orion_ft_mod_modulate_device": (i, [vp, vp, sz, vp, vp]),
        "orion_ft_mod_host": (i, [i, f, f, f, f, vp, vp]),
        "orion_ft_symbol_sequence": (i, [i, vp, vp]),
        "orion_ft_mod_tables": (i, [i, f, f, vp, vp, vp, vp]),
        "orion_ft_synth": (i, [i, f, vp, vp, sz, sz, sz, i, vp]),
        "orion_ft_synth_device": (i, [i, f, vp, vp, sz, sz, sz, i, vp, vp]),
        "orion_ft_demod": (i, [i, f, f, vp, sz, sz, vp, vp]),
        "orion_ft_demod_device": (i, [i, f, f, vp, sz, sz, vp, vp, vp]),
        "orion_ft_demod_host": (i, [i, f, f, vp, vp, vp]),
        "orion_psk31_tables": (i, [vp, vp, vp]),
        "orion_varicode_encode": (i, [C.c_uint8, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)]),
        "orion_varicode_decode": (i, [C.c_uint16, C.c_uint8]),
        "orion_varicode_encoder_new": (vp, []), "orion_varicode_encoder_free": (None, [vp]),
        "orion_varicode_encoder_push_preamble": (i, [vp, sz]), "orion_varicode_encoder_push_byte": (i, [vp, C.c_uint8]),
        "orion_varicode_encoder_push_postamble": (i, [vp, sz]), "orion_varicode_encoder_pending": (sz, [vp]),
        "orion_varicode_encoder_drain": (i, [vp, vp, sz, C.POINTER(sz)]),
        "orion_varicode_decoder_new": (vp, []), "orion_varicode_decoder_free": (None, [vp]),
        "orion_varicode_decoder_push_bits": (i, [vp, vp, sz]), "orion_varicode_decoder_pending": (sz, [vp]),
        "orion_varicode_decoder_pop_bytes": (i, [vp, vp, sz, C.POINTER(sz)]),
        "orion_conv_encode": (i, [vp, sz, vp]),
        "orion_psk31_viterbi": (i, [vp, sz, sz, vp]),
        "orion_psk31_viterbi_device": (i, [vp, sz, sz, vp, vp, sz, vp]),
        "orion_psk31_viterbi_work_bytes": (sz, [sz, sz]),
        "orion_psk31_viterbi_host": (i, [vp, sz, vp]), "orion_psk31_viterbi_hard_host": (i, [vp, sz, vp]),
        "orion_psk31_streaming_viterbi_new": (vp, []), "orion_psk31_streaming_viterbi_free": (None, [vp]),
        "orion_psk31_streaming_viterbi_feed": (i, [vp, vp, sz, vp, C.POINTER(sz)]),
        "orion_psk31_streaming_viterbi_flush": (i, [vp, vp, C.POINTER(sz)]),
        "orion_psk31_sps": (sz, [f]),
        "orion_psk31_synth": (i, [f, vp, vp, sz, sz, sz, i, vp]),
        "orion_psk31_synth_device": (i, [f, vp, vp, sz, sz, sz, i, vp, vp]),
        "orion_psk31_rotator_q64": (C.c_uint64, [f, f]),
        "orion_psk31_text_bits": (i, [vp, sz, sz, sz, vp, sz, C.POINTER(sz)]),
        "orion_psk31_mod_new": (vp, [i, f, f, f]), "orion_psk31_mod_free": (None, [vp]),
        "orion_psk31_mod_set_gain": (i, [vp, f]), "orion_psk31_mod_reset": (i, [vp]),
        "orion_psk31_mod_modulate_bits": (i, [vp, vp, sz, vp]),
        "orion_psk31_mod_modulate_bits_device": (i, [vp, vp, sz, vp, vp]),
        "orion_psk31_mod_modulate_batch": (i, [vp, vp, sz, sz, vp]),
        "orion_psk31_mod_modulate_batch_device": (i, [vp, vp, sz, sz, vp, vp]),
        "orion_psk31_mod_process": (i, [vp, vp, sz, vp, sz, C.POINTER(WorkReport)]),
        "orion_psk31_demod_new": (vp, [i, f, f, f, sz]), "orion_psk31_demod_free": (None, [vp]),
        "orion_psk31_demod_set_gain": (i, [vp, f]), "orion_psk31_demod_reset": (i, [vp]),
        "orion_psk31_demod_process": (i, [vp, vp, sz, vp, sz, C.POINTER(WorkReport)]),
        "orion_bpsk31_decide": (i, [vp, sz, vp]),
        "orion_psk31_demod_bank_new": (vp, [f, vp, sz, sz]), "orion_psk31_demod_bank_free": (None, [vp]),
        "orion_psk31_demod_bank_process": (i, [vp, vp, sz, sz, vp, sz, vp, vp]),
        "orion_psk31_demod_bank_process_device": (i, [vp, vp, sz, sz, vp, sz, vp, vp, vp]),
        "orion_psk31_demod_bank_reset": (i, [vp]), "orion_psk31_demod_bank_set_gain": (i, [vp, sz, f]),
        "orion_psk31_find_carriers_host": (i, [vp, sz, sz, sz, sz, f, sz, vp, vp]),
        "orion_psk31_sync_num_bins": (sz, [f, f]),
        "orion_psk31_find_carriers": (i, [vp, vp, sz, sz, sz, sz, f, sz, vp, vp]),
        "orion_psk31_find_carriers_device": (i, [vp, vp, sz, sz, sz, sz, f, sz, vp, vp, vp]),
        "orion_psk31_sync": (i, [vp, vp, sz, sz, f, f, f, sz, f, sz, sz, vp, vp, vp, vp]),
        "orion_psk31_sync_device": (i, [vp, vp, sz, sz, f, f, f, sz, f, sz, sz, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


_L = _load()


def _err() -> str:
    return (_L.orion_last_error() or b"").decode()


def _check(rc: int):
    if rc != 0:
        raise OrionError(f"orion_sdr: error {rc}: {_err()}")


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _taps_of(h, which: int) -> np.ndarray:
    n = C.c_size_t(0)
    _check(_L.orion_block_taps(h, which, None, 0, C.byref(n)))
    out = np.zeros(n.value, np.float32)
    _check(_L.orion_block_taps(h, which, _fptr(out), n.value, C.byref(n)))
    return out


_DT = {0: np.complex64, 1: np.float32}


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class _Block:
    """Shared Block contract (reference src/core.rs:12-22)."""

    def __init__(self, handle):
        if not handle:
            raise OrionError(f"orion_sdr: construction failed: {_err()}")
        self._h = handle
        self._in = _DT[_L.orion_block_in_type(handle)]
        self._out = _DT[_L.orion_block_out_type(handle)]
        self._nch = _L.orion_block_channels(handle)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _L is not None:  # at interpreter exit the module globals may already be gone
            _L.orion_block_free(h)
            self._h = None

    @property
    def name(self) -> str:
        return _L.orion_block_name(self._h).decode()

    def out_len(self, n: int) -> int:
        return _L.orion_block_out_len(self._h, n)

    def reset(self):
        _check(_L.orion_block_reset(self._h))

    def _validate(self, x: np.ndarray) -> np.ndarray:
        # python/tests/test_unit.py:86-127: wrong dtype / ndim / non-contiguous -> error
        if not isinstance(x, np.ndarray):
            raise TypeError(f"{type(self).__name__}.process expects a numpy array")
        if x.dtype != self._in:
            raise TypeError(f"{type(self).__name__}.process expects {np.dtype(self._in).name}, got {x.dtype}")
        want_ndim = 1 if self._nch == 1 else 2
        if x.ndim != want_ndim:
            raise ValueError(f"{type(self).__name__}.process expects a {want_ndim}-D array, got {x.ndim}-D")
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("array is not C-contiguous")
        if self._nch > 1 and x.shape[0] != self._nch:
            raise ValueError(f"expected {self._nch} channels, got {x.shape[0]}")
        return x

    def process_into(self, x: np.ndarray, out: np.ndarray) -> WorkReport:
        """Preallocated path (core.rs:19-21 process_into): honours out capacity."""
        x = self._validate(x)
        n = x.shape[-1]
        wr = WorkReport()
        _check(_L.orion_block_process(self._h, x.ctypes.data, n, out.ctypes.data, out.shape[-1], C.byref(wr)))
        return wr

    def process(self, x):
        if _is_torch(x):
            return self.process_device(x)
        x = self._validate(x)
        n = x.shape[-1]
        cap = self.out_len(n)
        out = np.empty((cap,) if self._nch == 1 else (self._nch, cap), self._out)
        wr = WorkReport()
        _check(_L.orion_block_process(self._h, x.ctypes.data, n, out.ctypes.data, cap, C.byref(wr)))
        if wr.out_written != cap:
            out = out[..., : wr.out_written].copy()
        return out

    def process_device(self, x, out=None, stream=None):
        """Device buffers (torch CUDA tensors). Asynchronous on `stream`
        (default: torch's current stream). Returns out (its first out_written samples)."""
        import torch

        if not x.is_cuda or not x.is_contiguous():
            raise ValueError("process_device needs a contiguous CUDA tensor")
        want = torch.complex64 if self._in is np.complex64 else torch.float32
        if x.dtype != want:
            raise TypeError(f"expected {want}, got {x.dtype}")
        n = x.shape[-1]
        cap = self.out_len(n)
        odt = torch.complex64 if self._out is np.complex64 else torch.float32
        if out is None:
            out = torch.empty((cap,) if self._nch == 1 else (self._nch, cap), dtype=odt, device=x.device)
        else:
            cap = out.shape[-1]
        s = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
        wr = WorkReport()
        _check(_L.orion_block_process_device(self._h, x.data_ptr(), n, out.data_ptr(), cap, s, C.byref(wr)))
        return out if wr.out_written == cap else out[..., : wr.out_written]

    def taps(self, which: int = 0) -> np.ndarray:
        return _taps_of(self._h, which)

    _OPTS = {"scan_path": 1, "mod_passes": 2, "nco_table": 3}

    def configure_option(self, option: str, value: int):
        """Engine options (no reference counterpart; include/orion_sdr_amd.h
        orion_block_configure): scan_path 0/1 (single pass / three-kernel scan),
        mod_passes 0/3, nco_table 0..2^28 (outputs of the reference's oscillator
        recurrence tabulated per tune; 0 = the closed-form ideal phasor)."""
        _check(_L.orion_block_configure(self._h, self._OPTS[option], int(value)))
        return self

    def status(self):
        """Raise OrionError if a kernel of this handle flagged a device-side failure
        (a cross-workgroup wait that timed out) since the last check (non-blocking;
        include/orion_sdr_amd.h orion_block_status)."""
        _check(_L.orion_block_status(self._h))


# ---- DSP primitives (src/dsp) -------------------------------------------------
class Rotator(_Block):
    """dsp/rotator.rs:16 Rotator::new(freq_hz, fs); process = rotate_block (:74-85)."""

    def __init__(self, freq_hz: float, fs: float):
        super().__init__(_L.orion_rotator_new(freq_hz, fs))

    def set_freq(self, freq_hz: float, fs: float):
        """rotator.rs:35-39: a new step; the phase continues (synchronizes the device)."""
        _check(_L.orion_rotator_set_freq(self._h, freq_hz, fs))

    def reset_phase(self):
        """rotator.rs:28-31: phasor back to 1 + j0."""
        _check(_L.orion_rotator_reset_phase(self._h))

    def next_cs_block(self, n: int) -> np.ndarray:
        """rotator.rs:44-68 next / next_cs, n times: complex64 phasors, advancing the
        same oscillator as process / mix_usb_block."""
        out = np.empty(int(n), np.complex64)
        _check(_L.orion_rotator_next_cs_block(self._h, out.ctypes.data, out.size))
        return out

    def mix_usb_block(self, x):
        """rotator.rs:88-94: I*cos + Q*sin on the same oscillator (complex64 -> float32).
        A torch CUDA tensor runs on the device path (torch's current stream)."""
        wr = WorkReport()
        if _is_torch(x):
            import torch

            if not x.is_cuda or not x.is_contiguous() or x.dtype != torch.complex64:
                raise ValueError("mix_usb_block needs a contiguous complex64 CUDA tensor")
            out = torch.empty(x.shape[-1], dtype=torch.float32, device=x.device)
            s = torch.cuda.current_stream(x.device).cuda_stream
            _check(_L.orion_rotator_mix_usb_block_device(self._h, x.data_ptr(), x.shape[-1], out.data_ptr(),
                                                        out.shape[0], s, C.byref(wr)))
            return out
        x = self._validate(x)
        out = np.empty(x.shape[-1], np.float32)
        _check(_L.orion_rotator_mix_usb_block(self._h, x.ctypes.data, x.shape[-1], out.ctypes.data, out.size,
                                              C.byref(wr)))
        return out


class Nco(_Block):
    """dsp/nco.rs:20 Nco::new(freq_hz, fs) as a block: process = mix_with_nco per
    sample (nco.rs:63-66, the non-FMA product)."""

    def __init__(self, freq_hz: float, fs: float):
        super().__init__(_L.orion_nco_new(freq_hz, fs))

    def set_freq(self, freq_hz: float):
        """nco.rs:33-38 (fs from the constructor); the phase continues."""
        _check(_L.orion_nco_set_freq(self._h, freq_hz))

    def next_cs_block(self, n: int) -> np.ndarray:
        """nco.rs:42-58 next_cs, n times: complex64 (cos, sin) of each step's phasor."""
        out = np.empty(int(n), np.complex64)
        _check(_L.orion_nco_next_cs_block(self._h, out.ctypes.data, out.size))
        return out


class Biquad(_Block):
    """dsp/iir.rs:15-41 Biquad::new(b0, b1, b2, a1, a2) (TDF-II); reset() = Biquad::reset."""

    def __init__(self, b0: float, b1: float, b2: float, a1: float, a2: float):
        super().__init__(_L.orion_biquad_new(b0, b1, b2, a1, a2))


class LpDcCascade(_Block):
    """dsp/iir.rs:111 LpDcCascade::design(fs, lp_fc, dc_cut_hz); process (:151-165), or
    process_mapped(x, f) (:170-186) with map "identity" / "sqrt" / "abs"
    (sqrt_map=True: "sqrt", the AM-PowerSqrt use)."""

    MAPS = {"identity": 0, "sqrt": 1, "abs": 2}

    def __init__(self, fs: float, lp_fc: float, dc_cut_hz: float, sqrt_map: bool = False, map: str | None = None):
        super().__init__(_L.orion_lp_dc_cascade_new(fs, lp_fc, dc_cut_hz))
        if sqrt_map:
            _check(_L.orion_lp_dc_cascade_set_sqrt_map(self._h, 1))
        if map is not None:
            self.set_map(map)

    def set_map(self, map: str):
        """process_mapped's f from the next call on (before the first call)."""
        if map not in self.MAPS:
            raise ValueError(f"LpDcCascade map must be one of {sorted(self.MAPS)}, got {map!r}")
        _check(_L.orion_lp_dc_cascade_set_map(self._h, self.MAPS[map]))
        return self


class FirDecimator(_Block):
    """dsp/decim.rs:24 FirDecimator::new(fs, m, cutoff_hz, trans_hz). channels>1: batched
    [nch, n] input (independent streams)."""

    def __init__(self, fs: float, m: int, cutoff_hz: float, trans_hz: float, channels: int = 1):
        h = (_L.orion_fir_decimator_new(fs, m, cutoff_hz, trans_hz) if channels == 1
             else _L.orion_fir_decimator_batch_new(fs, m, cutoff_hz, trans_hz, channels))
        super().__init__(h)


class FirLowpass(_Block):
    """dsp/fir.rs:16 FirLowpass::design(fs, pass_hz, trans_hz) (real f32 stream)."""

    def __init__(self, fs: float, pass_hz: float, trans_hz: float):
        super().__init__(_L.orion_fir_lowpass_new(fs, pass_hz, trans_hz))


class FirLowpassIq(_Block):
    """dsp/fir.rs:176-297. Use FirLowpassIq.design(...) or FirLowpassIq.from_taps(...)."""

    def __init__(self, handle):
        super().__init__(handle)

    @classmethod
    def design(cls, num_taps: int, cutoff_norm: float, stopband_db: float, channels: int = 1) -> "FirLowpassIq":
        """fir.rs:186-188; channels > 1: a batch of independent [channels, n] streams."""
        if channels == 1:
            return cls(_L.orion_fir_lowpass_iq_design(num_taps, cutoff_norm, stopband_db))
        return cls.from_taps(cls.design(num_taps, cutoff_norm, stopband_db).taps(), channels)

    @classmethod
    def from_taps(cls, taps, channels: int = 1) -> "FirLowpassIq":
        t = np.ascontiguousarray(taps, np.float32)
        if channels == 1:
            return cls(_L.orion_fir_lowpass_iq_from_taps(_fptr(t) if t.size else None, t.size))
        return cls(_L.orion_fir_lowpass_iq_batch_from_taps(_fptr(t) if t.size else None, t.size, channels))

    def num_taps(self) -> int:
        """fir.rs:210-212."""
        n = C.c_size_t(0)
        _check(_L.orion_fir_lowpass_iq_num_taps(self._h, C.byref(n)))
        return int(n.value)

    def group_delay(self) -> int:
        """fir.rs:216-218: (num_taps - 1) / 2."""
        d = C.c_size_t(0)
        _check(_L.orion_fir_lowpass_iq_group_delay(self._h, C.byref(d)))
        return int(d.value)

    def filter_aligned(self, io: np.ndarray) -> np.ndarray:
        """fir.rs:260-276, returns the filtered copy (time-aligned, same length)."""
        x = np.array(self._validate(io), copy=True)
        _check(_L.orion_fir_lowpass_iq_filter_aligned(self._h, x.ctypes.data, x.size))
        return x

    def filter_aligned_device(self, io, stream=None):
        """fir.rs:260-276 in place on a contiguous complex64 CUDA tensor (as the
        reference's `&mut [C32]`), asynchronous on `stream`. Returns io."""
        import torch

        if not io.is_cuda or not io.is_contiguous() or io.dtype != torch.complex64 or io.dim() != 1:
            raise ValueError("filter_aligned_device needs a contiguous 1-D complex64 CUDA tensor")
        s = stream if stream is not None else torch.cuda.current_stream(io.device).cuda_stream
        _check(_L.orion_fir_lowpass_iq_filter_aligned_device(self._h, io.data_ptr(), io.shape[0], s))
        return io


class LpCascade(_Block):
    """dsp/iir.rs:49 LpCascade::design(fs, fc) as an f32 stream block."""

    def __init__(self, fs: float, fc: float):
        super().__init__(_L.orion_lp_cascade_new(fs, fc))


class DcBlocker(_Block):
    """dsp/dc.rs:15 DcBlocker::new(fs, cut_hz)."""

    def __init__(self, fs: float, cut_hz: float):
        super().__init__(_L.orion_dc_blocker_new(fs, cut_hz))


# ---- demodulators (src/demodulate; PyO3 signatures src/python/demodulate.rs) ---
class CwEnvelopeDemod(_Block):
    def __init__(self, sample_rate: float, tone_hz: float, env_bw_hz: float):
        super().__init__(_L.orion_cw_envelope_demod_new(sample_rate, tone_hz, env_bw_hz))

    def set_gain(self, g: float):
        _check(_L.orion_cw_envelope_demod_set_gain(self._h, g))


class AmEnvelopeDemod(_Block):
    """abs_approx=True uses k1=0.9482, k2=0.3920 (src/python/demodulate.rs:46-53)."""

    def __init__(self, fs: float, audio_bw_hz: float, abs_approx: bool = False):
        super().__init__(_L.orion_am_envelope_demod_new(fs, audio_bw_hz))
        if abs_approx:
            _check(_L.orion_am_envelope_demod_with_abs_approx(self._h, 0.9482, 0.3920))

    def with_abs_approx(self, k1: float, k2: float) -> "AmEnvelopeDemod":
        _check(_L.orion_am_envelope_demod_with_abs_approx(self._h, k1, k2))
        return self


class SsbProductDemod(_Block):
    def __init__(self, fs: float, bfo_hz: float, audio_bw_hz: float, channels: int = 1):
        h = (_L.orion_ssb_product_demod_new(fs, bfo_hz, audio_bw_hz) if channels == 1
             else _L.orion_ssb_product_demod_batch_new(fs, bfo_hz, audio_bw_hz, channels))
        super().__init__(h)


class FmQuadratureDemod(_Block):
    def __init__(self, fs: float, dev_hz: float, audio_bw_hz: float):
        super().__init__(_L.orion_fm_quadrature_demod_new(fs, dev_hz, audio_bw_hz))

    def with_translate(self, freq_hz: float) -> "FmQuadratureDemod":
        _check(_L.orion_fm_quadrature_demod_with_translate(self._h, freq_hz))
        return self


class PmQuadratureDemod(_Block):
    def __init__(self, fs: float, k: float, audio_bw_hz: float):
        super().__init__(_L.orion_pm_quadrature_demod_new(fs, k, audio_bw_hz))


# ---- analog modulators (src/modulate): f32 audio -> complex64 IQ ----
class AgcRms(_Block):
    """dsp/agc.rs:20-31 AgcRms::new(fs, attack_ms, release_ms, target_rms): real audio AGC."""

    def __init__(self, fs: float, attack_ms: float, release_ms: float, target_rms: float):
        super().__init__(_L.orion_agc_rms_new(fs, attack_ms, release_ms, target_rms))


class AgcRmsIq(_Block):
    """dsp/agc.rs:93-106 AgcRmsIq::new(fs, attack_ms, release_ms, target_rms): one gain on I and Q."""

    def __init__(self, fs: float, attack_ms: float, release_ms: float, target_rms: float):
        super().__init__(_L.orion_agc_rms_iq_new(fs, attack_ms, release_ms, target_rms))


class AmDsbMod(_Block):
    """modulate/am.rs:20-36: carrier_level 1 -> full carrier (A3E), 0 -> DSB-SC."""

    def __init__(self, fs: float, rf_hz: float, carrier_level: float, modulation_index: float):
        super().__init__(_L.orion_am_dsb_mod_new(fs, rf_hz, carrier_level, modulation_index))

    def set_gain(self, g: float):
        _check(_L.orion_am_dsb_mod_set_gain(self._h, g))

    def set_clamp(self, on: bool):
        _check(_L.orion_am_dsb_mod_set_clamp(self._h, 1 if on else 0))


class FmPhaseAccumMod(_Block):
    """modulate/fm.rs:21-38 (deviation in Hz per unit input; rf_hz 0 for baseband)."""

    def __init__(self, sample_rate: float, deviation_hz: float, rf_hz: float = 0.0):
        super().__init__(_L.orion_fm_phase_accum_mod_new(sample_rate, deviation_hz, rf_hz))

    def set_deviation(self, deviation_hz: float):
        _check(_L.orion_fm_phase_accum_mod_set_deviation(self._h, deviation_hz))

    def set_gain(self, g: float):
        _check(_L.orion_fm_phase_accum_mod_set_gain(self._h, g))


class PmDirectPhaseMod(_Block):
    """modulate/pm.rs:17-47 (phase kp * x in radians; rf_hz 0 for baseband)."""

    def __init__(self, sample_rate: float, kp_rad_per_unit: float, rf_hz: float = 0.0):
        super().__init__(_L.orion_pm_direct_phase_mod_new(sample_rate, kp_rad_per_unit, rf_hz))

    def set_gain(self, g: float):
        _check(_L.orion_pm_direct_phase_mod_set_gain(self._h, g))

    def set_sensitivity(self, kp_rad_per_unit: float):
        _check(_L.orion_pm_direct_phase_mod_set_sensitivity(self._h, kp_rad_per_unit))


class CwKeyedMod(_Block):
    """modulate/cw.rs:21-87: keying envelope (0..1) -> keyed tone IQ."""

    def __init__(self, sample_rate: float, tone_hz: float, rise_ms: float, fall_ms: float):
        super().__init__(_L.orion_cw_keyed_mod_new(sample_rate, tone_hz, rise_ms, fall_ms))

    def set_gain(self, g: float):
        _check(_L.orion_cw_keyed_mod_set_gain(self._h, g))


class TxLowpass:
    """multicarrier/tx_lowpass.rs:88-195: the TX spectral-mask spec, its sizing helpers
    (the reference's f32 arithmetic, in the library) and apply() = filter_aligned of
    FirLowpassIq::design(num_taps, cutoff_norm, stopband_db) on the GPU."""

    def __init__(self, cutoff_norm: float, num_taps: int, stopband_db: float):
        self.cutoff_norm, self.num_taps, self.stopband_db = float(np.float32(cutoff_norm)), int(num_taps), \
            float(np.float32(stopband_db))

    def _spec(self):
        return C.byref(TxLowpassSpec(self.cutoff_norm, self.num_taps, self.stopband_db))

    @classmethod
    def for_null_band(cls, n_fft: int, occupied_half: int, num_taps: int, stopband_db: float) -> "TxLowpass":
        s = _L.orion_tx_lowpass_for_null_band(n_fft, occupied_half, num_taps, stopband_db)
        return cls(s.cutoff_norm, s.num_taps, s.stopband_db)

    @staticmethod
    def taps_for_null_band(n_fft: int, occupied_half: int, stopband_db: float) -> int:
        return int(_L.orion_tx_lowpass_taps_for_null_band(n_fft, occupied_half, stopband_db))

    def group_delay(self) -> int:
        return int(_L.orion_tx_lowpass_group_delay(self._spec()))

    def transition_norm(self) -> float:
        return float(_L.orion_tx_lowpass_transition_norm(self._spec()))

    def transition_fits(self, n_fft: int, occupied_half: int) -> bool:
        return bool(_L.orion_tx_lowpass_transition_fits(self._spec(), n_fft, occupied_half))

    def stopband_edge_norm(self) -> float:
        return float(_L.orion_tx_lowpass_stopband_edge_norm(self._spec()))

    def fits_guard(self, cp_len: int, roll_off: int, backoff: int) -> bool:
        return bool(_L.orion_tx_lowpass_fits_guard(self._spec(), cp_len, roll_off, backoff))

    def filter(self) -> "FirLowpassIq":
        return FirLowpassIq(_L.orion_tx_lowpass_filter(self._spec()))

    def apply(self, stream):
        """tx_lowpass.rs:192-195: filter_aligned across the whole stream. A numpy array
        is returned filtered (a copy); a contiguous complex64 CUDA tensor is filtered
        in place on the device."""
        f = self.filter()
        return f.filter_aligned_device(stream) if _is_torch(stream) else f.filter_aligned(stream)


class SsbPhasingMod(_Block):
    """modulate/ssb.rs:22-35."""

    def __init__(self, fs: float, audio_bw_hz: float, audio_if_hz: float, rf_hz: float = 0.0, usb: bool = True):
        super().__init__(_L.orion_ssb_phasing_mod_new(fs, audio_bw_hz, audio_if_hz, rf_hz, 1 if usb else 0))


class WbfmChain(_Block):
    """The WBFM chain of docs/demodulate.md:128-133, fused on the GPU.
    f_off: a float (one channel) or a sequence (one channel each; input [nch, n])."""

    def __init__(self, fs=10e6, f_off=1.5e6, m=8, dec_cutoff=200e3, dec_trans=79e3, dev_hz=75e3,
                 audio_bw=15e3, audio_pass=15e3, audio_trans=10e3):
        offs = np.atleast_1d(np.asarray(f_off, np.float32))
        p = WbfmParams(fs, float(offs[0]), dec_cutoff, dec_trans, dev_hz, audio_bw, audio_pass,
                       audio_trans, m)
        if np.ndim(f_off) == 0:
            h = _L.orion_wbfm_chain_new(C.byref(p))
        else:
            offs = np.ascontiguousarray(offs)
            h = _L.orion_wbfm_chain_batch_new(C.byref(p), _fptr(offs), offs.size)
        super().__init__(h)
        self.m = int(m)

    _PATHS = {"auto": 0, "segmented": 1, "split": 3, "graph": 4}

    def configure(self, path: str = "auto", max_segments: int = 0):
        """Engine tuning / tests (no reference counterpart): the kernel path and a
        cap on the segmented kernel's waves (include/orion_sdr_amd.h)."""
        _check(_L.orion_wbfm_chain_configure(self._h, self._PATHS[path], int(max_segments)))
        return self

    def seek(self, index: int):
        """Absolute index of the next input sample (the NCO phase origin);
        no reference counterpart (include/orion_sdr_amd.h orion_wbfm_chain_seek)."""
        _check(_L.orion_wbfm_chain_seek(self._h, int(index)))
        return self

    def process_shard(self, x_halo, start: int, halo_start: int):
        """One time shard of a stream (stream_shard): x_halo holds input
        samples [halo_start, stop). The handle is reset and sought to halo_start,
        runs the halo (which settles the decimator history, the discriminator's
        previous sample, the LpCascade state and the audio FIR history), and the
        audio of [start, stop) is returned: the same samples a single handle
        produces for the whole stream, up to the halo's settling residual."""
        self.reset()
        self.seek(halo_start)
        y = self.process(x_halo)
        return y[(start - halo_start) // self.m:]


# ---- time-sharded streams ----------------------------------------------
# Halo before a shard: 1024 audio samples at M = 8. The LpCascade forgets its
# zero start state within ~560 samples (||A^560|| < 1e-10 at 1.25 MHz, the host's
# own check uses ||A^896|| ~ 1e-16), the audio FIR then needs 124 settled
# samples, and the decimator 126 raw inputs; the rest is margin.
STREAM_HALO = 8192


def stream_shard(n: int, rank: int, world: int, m: int = 8, halo: int = STREAM_HALO):
    """Rank `rank` of `world`'s time slice of ONE n-sample stream: (start, stop,
    halo_start). Cuts fall on multiples of m (the decimator keeps inputs 0, m,
    2m, ... of every call, decim.rs:66-71), so the shards' outputs concatenate
    to the single-stream output; halo_start = max(0, start - halo)."""
    if not (0 <= rank < world) or n < 0 or halo % m:
        raise ValueError("stream_shard: bad rank/world/n/halo")
    units = n // m
    start = (units * rank // world) * m
    stop = n if rank == world - 1 else (units * (rank + 1) // world) * m
    return start, stop, max(0, start - halo)


# ---- chains (src/core.rs:24-109) and block graphs -------------------------------
class _Chain:
    """core.rs:24-109: a chain wraps one block and returns a new array per call.
    Deliberate divergence from the reference: the reference returns out[..n]
    (n = input length) even when the block wrote fewer samples (a decimator
    then leaks stale samples, core.rs:70-77); here the result is
    out[:out_written]."""

    _in = _out = None

    def __init__(self, block: _Block):
        if block._in is not self._in or block._out is not self._out:
            raise TypeError(f"{type(self).__name__} needs a {np.dtype(self._in).name} -> "
                            f"{np.dtype(self._out).name} block, got {block.name}")
        self.block = block

    def process(self, x):
        return self.block.process(x)

    process_ref = process

    def process_into(self, x: np.ndarray, out: np.ndarray) -> WorkReport:
        return self.block.process_into(x, out)


class AudioToIqChain(_Chain):
    """core.rs:24-53 (f32 -> cf32)."""
    _in, _out = np.float32, np.complex64


class IqToIqChain(_Chain):
    """core.rs:55-80 (cf32 -> cf32)."""
    _in, _out = np.complex64, np.complex64


class IqToAudioChain(_Chain):
    """core.rs:82-109 (cf32 -> f32)."""
    _in, _out = np.complex64, np.float32


class Graph:
    """A linear graph of blocks run back to back on the device: the input is
    staged to HBM once, every intermediate stays there (each stage's output is
    the next one's input, honouring out_written), and only the last output
    returns to the host. The user-composed chains of docs/demodulate.md:128-133
    (e.g. Rotator -> FirDecimator -> FmQuadratureDemod -> FirLowpass) run this
    way; blocks keep their streaming state across calls as usual."""

    def __init__(self, *blocks: _Block):
        if not blocks:
            raise ValueError("Graph needs at least one block")
        for a, b in zip(blocks, blocks[1:]):
            if a._out is not b._in:
                raise TypeError(f"{a.name} outputs {np.dtype(a._out).name}, {b.name} takes {np.dtype(b._in).name}")
        self.blocks = list(blocks)

    def process(self, x):
        import torch

        host = not _is_torch(x)
        if host:
            x = self.blocks[0]._validate(x)
            cur = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
        else:
            cur = x
        for b in self.blocks:
            cur = b.process_device(cur)
        return cur.cpu().numpy() if host else cur


# ---- designs (host) ----------------------------------------------------------
def fir_lowpass_design(fs: float, pass_hz: float, trans_hz: float) -> np.ndarray:
    n = _L.orion_fir_lowpass_design(fs, pass_hz, trans_hz, None, 0)
    t = np.zeros(n, np.float32)
    _L.orion_fir_lowpass_design(fs, pass_hz, trans_hz, _fptr(t), n)
    return t


def kaiser_lowpass_taps(num_taps: int, cutoff_norm: float, stopband_db: float) -> np.ndarray:
    n = _L.orion_kaiser_lowpass_taps(num_taps, cutoff_norm, stopband_db, None, 0)
    t = np.zeros(n, np.float32)
    _L.orion_kaiser_lowpass_taps(num_taps, cutoff_norm, stopband_db, _fptr(t), n)
    return t


def kaiser_transition_norm(num_taps: int, stopband_db: float) -> float:
    return _L.orion_kaiser_transition_norm(num_taps, stopband_db)


def kaiser_num_taps(transition_norm: float, stopband_db: float) -> int:
    return _L.orion_kaiser_num_taps(transition_norm, stopband_db)


def lp_cascade_design(fs: float, fc: float) -> np.ndarray:
    o = np.zeros(5, np.float32)
    _L.orion_lp_cascade_design(fs, fc, _fptr(o))
    return o


def diag_stream_read(x, stream: int = 0) -> int:
    """On-box bandwidth probe (no reference counterpart): one streaming read of the
    leading bytes of the device tensor x on `stream`; returns the bytes read."""
    nb = _L.orion_diag_stream_read_bytes(x.numel() * x.element_size())
    _check(_L.orion_diag_stream_read(C.c_void_p(x.data_ptr()), nb, C.c_void_p(stream)))
    return int(nb)


def diag_spin(stream: int, workgroups: int, lds_bytes: int, seconds: float):
    """Residency tests (no reference counterpart): `workgroups` one-wave workgroups each
    holding lds_bytes of LDS for `seconds` of wall clock, asynchronous on `stream`."""
    _check(_L.orion_diag_spin(C.c_void_p(stream), int(workgroups), int(lds_bytes), float(seconds)))


def diag_stream_create(n_cus: int = 0) -> int:
    """A HIP stream restricted to the first n_cus CUs (0: unrestricted); free it with
    diag_stream_destroy."""
    s = _L.orion_diag_stream_create(int(n_cus))
    if not s:
        raise OrionError(f"orion_sdr: stream creation failed: {_err()}")
    return int(s)


def diag_stream_destroy(stream: int):
    _check(_L.orion_diag_stream_destroy(C.c_void_p(stream)))


def device_cus() -> int:
    """Compute units of the current device."""
    return int(_L.orion_device_cus())


def set_spin_limit(polls: int):
    """Test-only: polls a cross-workgroup wait makes before it times out (process-wide;
    0 makes every such wait time out at once). include/orion_sdr_amd.h."""
    _L.orion_debug_set_spin_limit(int(polls))


def spin_limit() -> int:
    return int(_L.orion_debug_spin_limit())


def osc_table_phasors(freq_hz: float, fs: float, n: int, budget: int = 1 << 20):
    """Host only: the first n phasors of Rotator(freq_hz, fs) as the engine tabulates
    them (include/orion_sdr_amd.h orion_osc_table_phasors). Returns (phasors,
    cyc_start, cyc_len, n_tab)."""
    out = np.empty(int(n), np.complex64)
    cs, cl, nt = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(_L.orion_osc_table_phasors(freq_hz, fs, int(budget), out.ctypes.data, out.size, C.byref(cs),
                                      C.byref(cl), C.byref(nt)))
    return out, int(cs.value), int(cl.value), int(nt.value)


# ---- FT8 / FT4 frame sync (src/sync; src/python/ft8.rs) ------------------------
CANDIDATE_DTYPE = np.dtype([("time_sym", np.int32), ("freq_bin", np.uint32), ("score", np.float32)])
_PATTERNS = {"ft8": 0, "ft4": 1}
_WF_MODES = {"log": 0, "energy": 1}
SYNC_LLR = 174
LDPC_N = 174
# include/orion_sdr_amd.h orion_ldpc_result / orion_decode_pick
RESULT_DTYPE = np.dtype([("payload", np.uint8, (10,)), ("status", np.uint8), ("iterations", np.uint8),
                         ("errors", np.uint16), ("pad", np.uint16)])
PICK_DTYPE = np.dtype([("first_ok", np.int32), ("carrier_hz", np.float32), ("snr_db", np.float32), ("pad", np.uint32)])
_RULES = {"reference": 0, "sum_product": 1}


def _rule(rule) -> int:
    """A rule name, or a number passed through for the library to judge."""
    return _RULES[rule] if rule in _RULES else int(rule)


def sync_geometry(pattern: str, base_hz: float, max_hz: float, t_min: int, t_max: int):
    """Host only: (num_bins, wf_syms, wf_sample_start, sym_offset_adj, wf_t_max) of an
    ft8_sync / ft4_sync call (sync/ft8_sync.rs:99-131)."""
    g = (C.c_size_t * 5)()
    _check(_L.orion_sync_geometry(_PATTERNS[pattern], base_hz, max_hz, int(t_min), int(t_max), g))
    return tuple(int(v) for v in g)


class SyncEngine:
    """The FT8 / FT4 sync front end on the GPU (include/orion_sdr_amd.h orion_sync): a
    handle that keeps its step table, scratch waterfall and score map between calls.
    IQ is complex64, 1-D (one channel) or (nch, n); numpy arrays or torch CUDA tensors.
    The module-level compute_waterfall / find_candidates / ft8_sync / ft4_sync use one
    shared engine."""

    def __init__(self):
        h = _L.orion_sync_new()
        if not h:
            raise OrionError(f"orion_sdr: construction failed: {_err()}")
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _L is not None:
            _L.orion_sync_free(h)
            self._h = None

    def set_rows_per_lane(self, rows: int):
        """Engine tuning: symbol rows per lane of the waterfall kernel (1, 2, 4, 8; 0 = auto)."""
        _check(_L.orion_sync_set_rows_per_lane(self._h, int(rows)))
        return self

    @staticmethod
    def _iq(iq):
        """-> (array, nch, n, batched): a C-contiguous complex64 numpy array or CUDA tensor."""
        if _is_torch(iq):
            import torch

            if not iq.is_cuda or not iq.is_contiguous():
                raise ValueError("sync needs a contiguous CUDA tensor")
            if iq.dtype != torch.complex64:
                raise TypeError(f"expected torch.complex64, got {iq.dtype}")
        else:
            if not isinstance(iq, np.ndarray):
                raise TypeError("sync expects a numpy array or a torch CUDA tensor")
            if iq.dtype != np.complex64:
                raise TypeError(f"expected complex64, got {iq.dtype}")
            if not iq.flags["C_CONTIGUOUS"]:
                raise ValueError("array is not C-contiguous")
        if iq.ndim not in (1, 2):
            raise ValueError(f"expected a 1-D or (nch, n) array, got {iq.ndim}-D")
        if iq.ndim == 2 and iq.shape[0] < 1:
            raise ValueError("expected at least one channel")
        return iq, (1 if iq.ndim == 1 else iq.shape[0]), iq.shape[-1], iq.ndim == 2

    @staticmethod
    def _stream(x, stream):
        import torch

        return stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream

    def compute_waterfall(self, iq, fs, base_hz, tone_spacing_hz, samples_per_sym, num_syms, num_tones,
                          time_offset=0, mode="log", stream=None):
        """compute_waterfall (sync/waterfall.rs:73-119): mag (num_syms, num_tones) float32
        (with a leading nch axis for (nch, n) input). mode "log": ln(e + 1e-12); "energy":
        the Goertzel energy e itself."""
        iq, nch, n, batched = self._iq(iq)
        shape = (nch, num_syms, num_tones) if batched else (num_syms, num_tones)
        args = (float(fs), float(base_hz), float(tone_spacing_hz), int(samples_per_sym), int(num_syms),
                int(num_tones), int(time_offset), nch, n, _WF_MODES[mode])
        if _is_torch(iq):
            import torch

            mag = torch.empty(shape, dtype=torch.float32, device=iq.device)
            _check(_L.orion_waterfall_compute_device(self._h, iq.data_ptr(), *args, mag.data_ptr(),
                                                     self._stream(iq, stream)))
            return mag
        mag = np.empty(shape, np.float32)
        _check(_L.orion_waterfall_compute(self._h, iq.ctypes.data, *args, mag.ctypes.data))
        return mag

    @staticmethod
    def _wf(wf):
        """-> (CUDA tensor, nch, num_syms, num_tones, batched); numpy is uploaded."""
        import torch

        if not _is_torch(wf):
            wf = np.ascontiguousarray(wf, np.float32)
            wf = torch.from_numpy(wf).cuda()
        if not wf.is_cuda or not wf.is_contiguous() or wf.dtype != torch.float32:
            raise ValueError("waterfall: a contiguous float32 array or CUDA tensor")
        if wf.ndim not in (2, 3):
            raise ValueError(f"waterfall: (num_syms, num_tones) or (nch, num_syms, num_tones), got {wf.ndim}-D")
        return wf, (1 if wf.ndim == 2 else wf.shape[0]), wf.shape[-2], wf.shape[-1], wf.ndim == 3

    def find_candidates_device(self, wf, pattern, t_min, t_max, max_cand, stream=None):
        """The raw device call: (cand int32 tensor (nch, max_cand, 3) holding CANDIDATE_DTYPE
        records, count uint32-as-int32 tensor (nch,)), asynchronous on the stream."""
        import torch

        wf, nch, ns, nt, _ = self._wf(wf)
        cand = torch.empty((nch, max(int(max_cand), 1), 3), dtype=torch.int32, device=wf.device)
        count = torch.empty((nch,), dtype=torch.int32, device=wf.device)
        _check(_L.orion_costas_find_candidates_device(self._h, wf.data_ptr(), nch, ns, nt, _PATTERNS[pattern],
                                                      int(t_min), int(t_max), int(max_cand), cand.data_ptr(),
                                                      count.data_ptr(), self._stream(wf, stream)))
        return cand, count

    def find_candidates(self, wf, pattern, t_min, t_max, max_cand):
        """find_candidates (sync/costas.rs:125-174; pattern "ft8") / find_ft4_candidates
        (sync/ft4_sync.rs:122-163; "ft4") on a waterfall (numpy or CUDA tensor): a
        CANDIDATE_DTYPE record array, best first, in the reference's order among equal
        scores (a list of them, one per channel, for a 3-D waterfall)."""
        cand, count = self.find_candidates_device(wf, pattern, t_min, t_max, max_cand)
        c = cand.cpu().numpy().view(CANDIDATE_DTYPE)[..., 0]
        k = count.cpu().numpy()
        out = [c[ch, :k[ch]].copy() for ch in range(len(k))]
        return out if wf.ndim == 3 else out[0]

    def extract_llr(self, wf, pattern, cand):
        """extract_*_llr + normalise_llr (sync/ft8_sync.rs:170-246, ft4_sync.rs:227-292) of
        a CANDIDATE_DTYPE record array on a 2-D waterfall: float32 (len(cand), 174)."""
        import torch

        wf, nch, ns, nt, batched = self._wf(wf)
        if batched:
            raise ValueError("extract_llr: one channel at a time")
        cand = np.ascontiguousarray(cand, CANDIDATE_DTYPE)
        n = len(cand)
        if n == 0:
            return np.zeros((0, SYNC_LLR), np.float32)
        dc = torch.from_numpy(cand.view(np.int32).reshape(n, 3).copy()).to(wf.device)
        dn = torch.tensor([n], dtype=torch.int32, device=wf.device)
        llr = torch.empty((n, SYNC_LLR), dtype=torch.float32, device=wf.device)
        _check(_L.orion_sync_llr_device(wf.data_ptr(), 1, ns, nt, _PATTERNS[pattern], dc.data_ptr(), dn.data_ptr(), n,
                                        llr.data_ptr(), self._stream(wf, None)))
        return llr.cpu().numpy()

    def sync_raw(self, pattern, iq, fs, base_hz, max_hz, t_min, t_max, max_cand, stream=None):
        """ft8_sync / ft4_sync as arrays: (cand (nch, max_cand) CANDIDATE_DTYPE, count (nch,),
        llr (nch, max_cand, 174) float32), numpy whatever the input was."""
        iq, nch, n, _ = self._iq(iq)
        mc = int(max_cand)
        args = (nch, n, float(fs), float(base_hz), float(max_hz), int(t_min), int(t_max), mc)
        if _is_torch(iq):
            import torch

            fn = _L.orion_ft8_sync_device if pattern == "ft8" else _L.orion_ft4_sync_device
            cand = torch.empty((nch, max(mc, 1), 3), dtype=torch.int32, device=iq.device)
            count = torch.empty((nch,), dtype=torch.int32, device=iq.device)
            llr = torch.empty((nch, max(mc, 1), SYNC_LLR), dtype=torch.float32, device=iq.device)
            _check(fn(self._h, iq.data_ptr(), *args, cand.data_ptr(), count.data_ptr(), llr.data_ptr(),
                      self._stream(iq, stream)))
            return (cand.cpu().numpy().view(CANDIDATE_DTYPE)[..., 0], count.cpu().numpy().view(np.uint32),
                    llr.cpu().numpy())
        fn = _L.orion_ft8_sync if pattern == "ft8" else _L.orion_ft4_sync
        cand = np.zeros((nch, max(mc, 1)), CANDIDATE_DTYPE)
        count = np.zeros(nch, np.uint32)
        llr = np.zeros((nch, max(mc, 1), SYNC_LLR), np.float32)
        _check(fn(self._h, iq.ctypes.data, *args, cand.ctypes.data, count.ctypes.data, llr.ctypes.data))
        return cand, count, llr

    def _sync(self, pattern, iq, *a):
        cand, count, llr = self.sync_raw(pattern, iq, *a)
        out = [[{"time_sym": int(cand[ch, k]["time_sym"]), "freq_bin": int(cand[ch, k]["freq_bin"]),
                 "score": float(cand[ch, k]["score"]), "llr": llr[ch, k].copy()} for k in range(int(count[ch]))]
               for ch in range(len(count))]
        return out

    def ft8_sync(self, iq, fs, base_hz, max_hz, t_min, t_max, max_cand):
        """ft8_sync (sync/ft8_sync.rs:90-159; src/python/ft8.rs): list[dict] with keys
        time_sym, freq_bin, score, llr (float32[174]), best first. iq: 1-D."""
        if np.ndim(iq) != 1:
            raise ValueError("ft8_sync expects a 1-D array (ft8_sync_batch takes (nch, n))")
        return self._sync("ft8", iq, fs, base_hz, max_hz, t_min, t_max, max_cand)[0]

    def ft4_sync(self, iq, fs, base_hz, max_hz, t_min, t_max, max_cand):
        """ft4_sync (sync/ft4_sync.rs:65-117): as ft8_sync."""
        if np.ndim(iq) != 1:
            raise ValueError("ft4_sync expects a 1-D array (ft4_sync_batch takes (nch, n))")
        return self._sync("ft4", iq, fs, base_hz, max_hz, t_min, t_max, max_cand)[0]

    def ft8_sync_batch(self, iq, fs, base_hz, max_hz, t_min, t_max, max_cand):
        """ft8_sync of every row of iq (nch, n) in one device call: a list per channel."""
        if np.ndim(iq) != 2:
            raise ValueError("ft8_sync_batch expects an (nch, n) array")
        return self._sync("ft8", iq, fs, base_hz, max_hz, t_min, t_max, max_cand)

    def ft4_sync_batch(self, iq, fs, base_hz, max_hz, t_min, t_max, max_cand):
        if np.ndim(iq) != 2:
            raise ValueError("ft4_sync_batch expects an (nch, n) array")
        return self._sync("ft4", iq, fs, base_hz, max_hz, t_min, t_max, max_cand)


    def decode_raw(self, pattern, iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule="reference", max_iter=20,
                   stream=None):
        """ft8_decode / ft4_decode as arrays: (cand, count, llr, results (nch, max_cand)
        RESULT_DTYPE, pick (nch,) PICK_DTYPE), numpy whatever the input was. One device call:
        sync, the LDPC + CRC decode of every candidate and the pick, on one stream."""
        iq, nch, n, _ = self._iq(iq)
        mc = int(max_cand)
        args = (nch, n, float(fs), float(base_hz), float(max_hz), int(t_min), int(t_max), mc, _rule(rule), int(max_iter))
        if _is_torch(iq):
            import torch

            fn = _L.orion_ft8_decode_device if pattern == "ft8" else _L.orion_ft4_decode_device
            cand = torch.empty((nch, max(mc, 1), 3), dtype=torch.int32, device=iq.device)
            count = torch.empty((nch,), dtype=torch.int32, device=iq.device)
            llr = torch.empty((nch, max(mc, 1), SYNC_LLR), dtype=torch.float32, device=iq.device)
            res = torch.empty((nch, max(mc, 1), 4), dtype=torch.int32, device=iq.device)
            pick = torch.empty((nch, 4), dtype=torch.int32, device=iq.device)
            _check(fn(self._h, iq.data_ptr(), *args, cand.data_ptr(), count.data_ptr(), llr.data_ptr(), res.data_ptr(),
                      pick.data_ptr(), self._stream(iq, stream)))
            return (cand.cpu().numpy().view(CANDIDATE_DTYPE)[..., 0], count.cpu().numpy().view(np.uint32),
                    llr.cpu().numpy(), res.cpu().numpy().view(RESULT_DTYPE)[..., 0],
                    pick.cpu().numpy().view(PICK_DTYPE)[..., 0])
        fn = _L.orion_ft8_decode if pattern == "ft8" else _L.orion_ft4_decode
        cand = np.zeros((nch, max(mc, 1)), CANDIDATE_DTYPE)
        count = np.zeros(nch, np.uint32)
        llr = np.zeros((nch, max(mc, 1), SYNC_LLR), np.float32)
        res = np.zeros((nch, max(mc, 1)), RESULT_DTYPE)
        pick = np.zeros(nch, PICK_DTYPE)
        _check(fn(self._h, iq.ctypes.data, *args, cand.ctypes.data, count.ctypes.data, llr.ctypes.data,
                  res.ctypes.data, pick.ctypes.data))
        return cand, count, llr, res, pick

    def _decode(self, pattern, iq, *a, **kw):
        cand, count, llr, res, pick = self.decode_raw(pattern, iq, *a, **kw)
        out = []
        for ch in range(len(count)):
            k = int(count[ch])
            fo = int(pick[ch]["first_ok"])
            out.append({
                "candidates": [{"time_sym": int(c["time_sym"]), "freq_bin": int(c["freq_bin"]), "score": float(c["score"])}
                               for c in cand[ch, :k]],
                "llr": llr[ch, :k].copy(), "results": res[ch, :k].copy(), "first_ok": fo,
                "payload": res[ch, fo]["payload"].tobytes() if fo >= 0 else None,
                "carrier_hz": float(pick[ch]["carrier_hz"]) if fo >= 0 else None,
                "snr_db": float(pick[ch]["snr_db"]) if fo >= 0 else None})
        return out

    def ft8_decode(self, iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule="reference", max_iter=20):
        """ft8_sync, then Ft8Codec::decode_soft of every candidate on the device, and the
        reference stream decoder's pick (codec/ft8.rs:252-323): a dict with candidates,
        llr, results (RESULT_DTYPE), first_ok (the first candidate with status 2, or -1)
        and its payload (bytes), carrier_hz and snr_db (None when first_ok is -1). iq: 1-D."""
        if np.ndim(iq) != 1:
            raise ValueError("ft8_decode expects a 1-D array (ft8_decode_batch takes (nch, n))")
        return self._decode("ft8", iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule=rule, max_iter=max_iter)[0]

    def ft4_decode(self, iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule="reference", max_iter=20):
        if np.ndim(iq) != 1:
            raise ValueError("ft4_decode expects a 1-D array (ft4_decode_batch takes (nch, n))")
        return self._decode("ft4", iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule=rule, max_iter=max_iter)[0]

    def ft8_decode_batch(self, iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule="reference", max_iter=20):
        """ft8_decode of every row of iq (nch, n) in one device call: a dict per channel."""
        if np.ndim(iq) != 2:
            raise ValueError("ft8_decode_batch expects an (nch, n) array")
        return self._decode("ft8", iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule=rule, max_iter=max_iter)

    def ft4_decode_batch(self, iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule="reference", max_iter=20):
        if np.ndim(iq) != 2:
            raise ValueError("ft4_decode_batch expects an (nch, n) array")
        return self._decode("ft4", iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule=rule, max_iter=max_iter)


_SYNC = None


def _sync_engine() -> SyncEngine:
    global _SYNC
    if _SYNC is None:
        _SYNC = SyncEngine()
    return _SYNC


def compute_waterfall(iq, fs, base_hz, tone_spacing_hz, samples_per_sym, num_syms, num_tones, time_offset=0,
                      mode="log"):
    return _sync_engine().compute_waterfall(iq, fs, base_hz, tone_spacing_hz, samples_per_sym, num_syms, num_tones,
                                            time_offset, mode)


def find_candidates(wf, pattern, t_min, t_max, max_cand):
    return _sync_engine().find_candidates(wf, pattern, t_min, t_max, max_cand)


def ft8_sync(iq, fs, base_hz, max_hz, t_min, t_max, max_cand):
    return _sync_engine().ft8_sync(iq, fs, base_hz, max_hz, t_min, t_max, max_cand)


def ft4_sync(iq, fs, base_hz, max_hz, t_min, t_max, max_cand):
    return _sync_engine().ft4_sync(iq, fs, base_hz, max_hz, t_min, t_max, max_cand)


def ft8_sync_batch(iq, fs, base_hz, max_hz, t_min, t_max, max_cand):
    return _sync_engine().ft8_sync_batch(iq, fs, base_hz, max_hz, t_min, t_max, max_cand)


def ft4_sync_batch(iq, fs, base_hz, max_hz, t_min, t_max, max_cand):
    return _sync_engine().ft4_sync_batch(iq, fs, base_hz, max_hz, t_min, t_max, max_cand)


def ft8_decode(iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule="reference", max_iter=20):
    return _sync_engine().ft8_decode(iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule, max_iter)


def ft4_decode(iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule="reference", max_iter=20):
    return _sync_engine().ft4_decode(iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule, max_iter)


def ft8_decode_batch(iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule="reference", max_iter=20):
    return _sync_engine().ft8_decode_batch(iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule, max_iter)


def ft4_decode_batch(iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule="reference", max_iter=20):
    return _sync_engine().ft4_decode_batch(iq, fs, base_hz, max_hz, t_min, t_max, max_cand, rule, max_iter)


# ---- FT8 / FT4 channel codec: LDPC(174,91) + CRC-14 (src/codec; src/python/ft8.rs) ----
def ft_crc14(message: bytes, num_bits: int) -> int:
    """ft8_crc14 (codec/crc.rs:37-54) over the first num_bits bits of message."""
    message = bytes(message)
    if num_bits < 0 or num_bits > 8 * len(message):
        raise ValueError("num_bits beyond the message")
    return int(_L.orion_ft_crc14(message, int(num_bits)))


def ldpc_tables():
    """Host only: the code's edge list as the library states it and the tables it derives:
    (edges (522, 2) uint8 [check, bit], row_start (84,) uint16, bit_check (174, 3) uint8,
    generator (83, 12) uint8)."""
    edges = np.zeros((522, 2), np.uint8)
    row_start = np.zeros(84, np.uint16)
    bit_check = np.zeros((LDPC_N, 3), np.uint8)
    gen = np.zeros((83, 12), np.uint8)
    _check(_L.orion_ldpc_tables(edges.ctypes.data, row_start.ctypes.data, bit_check.ctypes.data, gen.ctypes.data))
    return edges, row_start, bit_check, gen


def _llr174(llr) -> np.ndarray:
    if not isinstance(llr, np.ndarray) or llr.dtype != np.float32 or llr.shape != (LDPC_N,):
        raise ValueError("expected a float32 array of 174 LLRs")
    return np.ascontiguousarray(llr)


def ldpc_decode_host(llr, protocol="ft8", rule="reference", max_iter=20):
    """The library's scalar decoder (host only; what the kernel is held to) on one
    codeword: (result: a RESULT_DTYPE record, plain uint8[174])."""
    llr = _llr174(llr)
    res = np.zeros(1, RESULT_DTYPE)
    plain = np.zeros(LDPC_N, np.uint8)
    _check(_L.orion_ldpc_decode_host(llr.ctypes.data, _PATTERNS[protocol], _rule(rule), int(max_iter), res.ctypes.data,
                                     plain.ctypes.data))
    return res[0], plain


def ldpc_decode_batch(llr, protocol, rule="reference", max_iter=20, return_plain=False, count=None, stream=None):
    """LDPC(174,91) belief propagation + CRC-14 of a batch of codewords on the GPU, one
    wave64 workgroup each: llr float32 [..., 174] (numpy array or torch CUDA tensor) ->
    a RESULT_DTYPE array of shape [...] (numpy either way), and with return_plain the best
    hard decisions uint8 [..., 174] as well. count (optional, uint32 (nch,)): llr is the
    (nch, max_cand, 174) layout ft8_sync writes; slots at or past count[ch] are not
    decoded and give all-zero records."""
    tl = _is_torch(llr)
    if tl:
        import torch

        if not llr.is_cuda or not llr.is_contiguous() or llr.dtype != torch.float32:
            raise ValueError("ldpc_decode_batch needs a contiguous float32 CUDA tensor")
    else:
        if not isinstance(llr, np.ndarray) or llr.dtype != np.float32:
            raise ValueError("ldpc_decode_batch expects a float32 numpy array or torch CUDA tensor")
        llr = np.ascontiguousarray(llr)
    if llr.ndim < 1 or llr.shape[-1] != LDPC_N:
        raise ValueError(f"expected LLRs of shape [..., 174], got {tuple(llr.shape)}")
    shape = tuple(llr.shape[:-1])
    n = int(np.prod(shape, dtype=np.int64))
    mc = 0
    if count is not None:
        if llr.ndim != 3:
            raise ValueError("count goes with LLRs of shape (nch, max_cand, 174)")
        mc = int(shape[1])
    proto, rl, mi = _PATTERNS[protocol], _rule(rule), int(max_iter)
    if tl:
        import torch

        res = torch.empty(shape + (4,), dtype=torch.int32, device=llr.device)
        plain = torch.empty(shape + (LDPC_N,), dtype=torch.uint8, device=llr.device) if return_plain else None
        dcount = None
        if count is not None:
            dcount = count if _is_torch(count) else torch.from_numpy(np.ascontiguousarray(count, np.uint32).view(np.int32)).to(llr.device)
            if dcount.numel() != shape[0] or not dcount.is_cuda or dcount.element_size() != 4:
                raise ValueError("count: one 32-bit entry per channel")
        _check(_L.orion_ldpc_decode_device(llr.data_ptr(), n, dcount.data_ptr() if dcount is not None else None, mc, proto,
                                           rl, mi, res.data_ptr(), plain.data_ptr() if return_plain else None,
                                           SyncEngine._stream(llr, stream)))
        out = res.cpu().numpy().view(RESULT_DTYPE)[..., 0]
        return (out, plain.cpu().numpy()) if return_plain else out
    res = np.zeros(shape, RESULT_DTYPE)
    plain = np.zeros(shape + (LDPC_N,), np.uint8) if return_plain else None
    hcount = None
    if count is not None:
        hcount = np.ascontiguousarray(count, np.uint32)
        if hcount.shape != (shape[0],):
            raise ValueError("count: one entry per channel")
    _check(_L.orion_ldpc_decode(llr.ctypes.data, n, hcount.ctypes.data if hcount is not None else None, mc, proto, rl, mi,
                                res.ctypes.data, plain.ctypes.data if return_plain else None))
    return (res, plain) if return_plain else res


class _FtCodec:
    """Ft8Codec / Ft4Codec (src/python/ft8.rs:94-160, 236-300): static encode, decode_hard
    and decode_soft of one frame, on the library's host scalar decoder (one codeword is
    not worth a launch). rule and max_iter are keyword extras; the defaults are the
    reference's."""
    _protocol = "ft8"
    _tones = 58

    @classmethod
    def encode(cls, payload) -> np.ndarray:
        payload = bytes(payload)
        if len(payload) != 10:
            raise ValueError("payload must be 10 bytes")
        tones = np.zeros(cls._tones, np.uint8)
        fn = _L.orion_ft8_encode if cls._protocol == "ft8" else _L.orion_ft4_encode
        _check(fn(payload, tones.ctypes.data, None))
        return tones

    @classmethod
    def frame_to_llr_hard(cls, tones) -> np.ndarray:
        if not isinstance(tones, np.ndarray) or tones.dtype != np.uint8 or tones.shape != (cls._tones,):
            raise ValueError(f"expected a uint8 array of {cls._tones} tones")
        tones = np.ascontiguousarray(tones)
        llr = np.zeros(LDPC_N, np.float32)
        _check(_L.orion_ft_frame_to_llr_hard(_PATTERNS[cls._protocol], tones.ctypes.data, llr.ctypes.data))
        return llr

    @classmethod
    def decode_hard(cls, tones, *, rule="reference", max_iter=20):
        return cls.decode_soft(cls.frame_to_llr_hard(tones), rule=rule, max_iter=max_iter)

    @classmethod
    def decode_soft(cls, llr, *, rule="reference", max_iter=20):
        res, _ = ldpc_decode_host(_llr174(llr), cls._protocol, rule, max_iter)
        return res["payload"].tobytes() if res["status"] == 2 else None


class Ft8Codec(_FtCodec):
    _protocol, _tones = "ft8", 58


class Ft4Codec(_FtCodec):
    _protocol, _tones = "ft4", 87


# ---- FT8 / FT4 modulators, slot synthesis and hard demodulators ---------------------------
FT8_FRAME_LEN = 79 * 1920
FT4_FRAME_LEN = 105 * 576
SIGNAL_DTYPE = np.dtype([("channel", np.uint32), ("pad", np.uint32), ("offset", np.int64), ("base_hz", np.float32),
                         ("gain", np.float32)])
_FT = {"ft8": (58, 79, 8, FT8_FRAME_LEN), "ft4": (87, 105, 4, FT4_FRAME_LEN)}  # data, total, tones, frame length


def _ft_tones(tones, ndata, batched_ok=True):
    """-> (C-contiguous uint8 array, nframes, batched); ValueError as the PyO3 classes."""
    if not isinstance(tones, np.ndarray) or tones.dtype != np.uint8:
        raise ValueError(f"expected a uint8 array of {ndata} tones")
    if tones.ndim == 1 and tones.shape[0] == ndata:
        return np.ascontiguousarray(tones), 1, False
    if batched_ok and tones.ndim == 2 and tones.shape[1] == ndata:
        return np.ascontiguousarray(tones), tones.shape[0], True
    raise ValueError(f"expected {ndata} tones (or an (F, {ndata}) array), got shape {tuple(tones.shape)}")


def _ft_arg(rc: int):
    """A bad argument (a tone out of range, a channel >= nch) is a ValueError here."""
    if rc == -3:
        raise ValueError(f"orion_sdr: {_err()}")
    _check(rc)


class _FtMod:
    """Ft8Mod / Ft4Mod (src/python/ft8.rs; modulate/ft8.rs:48-156, ft4.rs:51-173): data tones
    -> one frame of complex64 IQ, on the GPU. The device generates the closed form of the
    reference's own f32 tone steps, which follows the reference's phasor recurrence to its
    rounding drift (about 1e-4 over a frame); modulate_host is the recurrence itself, bit
    for bit, on the host."""
    _protocol = "ft8"

    def __init__(self, fs: float, base_hz: float, rf_hz: float = 0.0, gain: float = 1.0):
        self._args = (float(fs), float(base_hz), float(rf_hz), float(gain))
        h = _L.orion_ft_mod_new(_PATTERNS[self._protocol], *self._args)
        if not h:
            raise OrionError(f"orion_sdr: construction failed: {_err()}")
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _L is not None:
            _L.orion_ft_mod_free(h)
            self._h = None

    def modulate(self, tones, device=False, stream=None):
        """tones uint8 [58 | 87] -> complex64 [frame_len]; (F, 58 | 87) -> (F, frame_len). A new
        array per call. device=True: a torch CUDA tensor, filled on torch's current stream."""
        ndata, _, _, flen = _FT[self._protocol]
        tones, nf, batched = _ft_tones(tones, ndata)
        shape = (nf, flen) if batched else (flen,)
        if device:
            import torch

            out = torch.empty(shape, dtype=torch.complex64, device="cuda")
            _ft_arg(_L.orion_ft_mod_modulate_device(self._h, tones.ctypes.data, nf, out.data_ptr(),
                                                    SyncEngine._stream(out, stream)))
            return out
        out = np.empty(shape, np.complex64)
        _ft_arg(_L.orion_ft_mod_modulate(self._h, tones.ctypes.data, nf, out.ctypes.data))
        return out

    def modulate_host(self, tones) -> np.ndarray:
        """The reference's own samples (its scalar recurrence, on the host)."""
        ndata, _, _, flen = _FT[self._protocol]
        tones, _, _ = _ft_tones(tones, ndata, batched_ok=False)
        out = np.empty(flen, np.complex64)
        _ft_arg(_L.orion_ft_mod_host(_PATTERNS[self._protocol], *self._args, tones.ctypes.data, out.ctypes.data))
        return out

    @classmethod
    def symbol_sequence(cls, tones) -> np.ndarray:
        """build_symbol_sequence: the 79 | 105 frame symbols, sync (and FT4 ramp) symbols included."""
        ndata, total, _, _ = _FT[cls._protocol]
        tones, _, _ = _ft_tones(tones, ndata, batched_ok=False)
        syms = np.zeros(total, np.uint8)
        _ft_arg(_L.orion_ft_symbol_sequence(_PATTERNS[cls._protocol], tones.ctypes.data, syms.ctypes.data))
        return syms

    def tables(self, tones=None):
        """(w complex64 [8 | 4], step uint64 [8 | 4], enter uint64 [79 | 105] or None): the f32
        step phasors, their angles as Q0.64 turns and the phase entering each symbol."""
        ndata, total, nt, _ = _FT[self._protocol]
        w = np.zeros(nt, np.complex64)
        step = np.zeros(nt, np.uint64)
        enter = None
        tp = None
        if tones is not None:
            tones, _, _ = _ft_tones(tones, ndata, batched_ok=False)
            enter = np.zeros(total, np.uint64)
            tp = tones.ctypes.data
        _ft_arg(_L.orion_ft_mod_tables(_PATTERNS[self._protocol], self._args[0], self._args[1], tp, w.ctypes.data,
                                       step.ctypes.data, enter.ctypes.data if enter is not None else None))
        return w, step, enter


class Ft8Mod(_FtMod):
    _protocol = "ft8"


class Ft4Mod(_FtMod):
    _protocol = "ft4"


class _FtDemod:
    """Ft8Demod / Ft4Demod (src/python/ft8.rs; demodulate/ft8.rs:25-126, ft4.rs): the argmax
    tone of every symbol's correlator energies, sync positions dropped; the reference's
    arithmetic bit for bit. IQ: complex64, 1-D or (F, n) with n >= a frame (only the first
    frame length of a row is read); a numpy array or a torch CUDA tensor."""
    _protocol = "ft8"

    def __init__(self, fs: float, base_hz: float):
        self._args = (float(fs), float(base_hz))

    def _run(self, iq, want_energies, stream=None):
        ndata, total, nt, flen = _FT[self._protocol]
        try:
            iq, nf, n, batched = SyncEngine._iq(iq)
        except TypeError as e:
            raise ValueError(str(e)) from None
        if n < flen:
            raise ValueError(f"expected at least {flen} samples per frame, got {n}")
        proto = _PATTERNS[self._protocol]
        tshape = (nf, ndata) if batched else (ndata,)
        eshape = (nf, total, nt) if batched else (total, nt)
        if _is_torch(iq):
            import torch

            tones = torch.empty(tshape, dtype=torch.uint8, device=iq.device)
            en = torch.empty(eshape, dtype=torch.float32, device=iq.device) if want_energies else None
            _ft_arg(_L.orion_ft_demod_device(proto, *self._args, iq.data_ptr(), nf, n, tones.data_ptr(),
                                             en.data_ptr() if want_energies else None, SyncEngine._stream(iq, stream)))
            return tones.cpu().numpy(), (en.cpu().numpy() if want_energies else None)
        tones = np.zeros(tshape, np.uint8)
        en = np.zeros(eshape, np.float32) if want_energies else None
        _ft_arg(_L.orion_ft_demod(proto, *self._args, iq.ctypes.data, nf, n, tones.ctypes.data,
                                  en.ctypes.data if want_energies else None))
        return tones, en

    def demodulate(self, iq) -> np.ndarray:
        """-> uint8 [58 | 87], or (F, 58 | 87) for (F, n) input (numpy either way)."""
        return self._run(iq, False)[0]

    def energies(self, iq) -> np.ndarray:
        """Every correlator energy: float32 (79 | 105, 8 | 4), with a leading F axis for (F, n)."""
        return self._run(iq, True)[1]

    def demodulate_host(self, iq, return_energies=False):
        """The library's scalar demodulator (host only; what the kernel is held to), one frame."""
        ndata, total, nt, flen = _FT[self._protocol]
        if not isinstance(iq, np.ndarray) or iq.dtype != np.complex64 or iq.ndim != 1 or len(iq) < flen:
            raise ValueError(f"expected a 1-D complex64 array of at least {flen} samples")
        iq = np.ascontiguousarray(iq)
        tones = np.zeros(ndata, np.uint8)
        en = np.zeros((total, nt), np.float32)
        _ft_arg(_L.orion_ft_demod_host(_PATTERNS[self._protocol], *self._args, iq.ctypes.data, tones.ctypes.data,
                                       en.ctypes.data))
        return (tones, en) if return_energies else tones


class Ft8Demod(_FtDemod):
    _protocol = "ft8"


class Ft4Demod(_FtDemod):
    _protocol = "ft4"


def _ft_synth(protocol, signals, tones, n, nch, fs, out, accumulate, device, stream):
    ndata = _FT[protocol][0]
    if not isinstance(signals, np.ndarray) or signals.dtype != SIGNAL_DTYPE or signals.ndim != 1:
        raise ValueError("signals: a 1-D array of SIGNAL_DTYPE")
    signals = np.ascontiguousarray(signals)
    nsig = len(signals)
    if not isinstance(tones, np.ndarray) or tones.dtype != np.uint8 or tones.shape != (nsig, ndata):
        raise ValueError(f"tones: a uint8 array of shape ({nsig}, {ndata})")
    tones = np.ascontiguousarray(tones)
    n, nch = int(n), int(nch)
    if n < 0 or nch < 1:
        raise ValueError("n >= 0 and nch >= 1")
    proto = _PATTERNS[protocol]
    if out is not None:
        if tuple(out.shape) != (nch, n):
            raise ValueError(f"out: expected shape ({nch}, {n}), got {tuple(out.shape)}")
    elif accumulate:
        raise ValueError("accumulate needs out")
    if (out is not None and _is_torch(out)) or (out is None and device):
        import torch

        if out is None:
            out = torch.empty((nch, n), dtype=torch.complex64, device="cuda")
        elif not out.is_cuda or not out.is_contiguous() or out.dtype != torch.complex64:
            raise ValueError("out: a contiguous complex64 CUDA tensor")
        _ft_arg(_L.orion_ft_synth_device(proto, float(fs), signals.ctypes.data, tones.ctypes.data, nsig, nch, n,
                                         1 if accumulate else 0, out.data_ptr(), SyncEngine._stream(out, stream)))
        return out
    if out is None:
        out = np.empty((nch, n), np.complex64)
    elif not isinstance(out, np.ndarray) or out.dtype != np.complex64 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("out: a C-contiguous complex64 array")
    _ft_arg(_L.orion_ft_synth(proto, float(fs), signals.ctypes.data, tones.ctypes.data, nsig, nch, n,
                              1 if accumulate else 0, out.ctypes.data))
    return out


def ft8_synth(signals, tones, n, nch=1, fs=12000.0, out=None, accumulate=False, device=False, stream=None):
    """Slot synthesis on the GPU: (nch, n) complex64 holding every signal's FT8 frame (as
    Ft8Mod(fs, base_hz, 0, gain).modulate gives it) at its offset in its channel, clipped to
    the channel, a channel's signals summed in list order (bit-reproducible). signals: a
    SIGNAL_DTYPE array (channel, offset, base_hz, gain); tones uint8 (nsig, 58). out: a numpy
    array or torch CUDA tensor to fill (accumulate: to add to); device=True: a new CUDA
    tensor, filled on torch's current stream."""
    return _ft_synth("ft8", signals, tones, n, nch, fs, out, accumulate, device, stream)


def ft4_synth(signals, tones, n, nch=1, fs=12000.0, out=None, accumulate=False, device=False, stream=None):
    """ft8_synth for FT4 frames: tones uint8 (nsig, 87)."""
    return _ft_synth("ft4", signals, tones, n, nch, fs, out, accumulate, device, stream)


# ---- PSK31 channel code: Varicode and QPSK31's rate 1/2, K = 5 code (src/codec) -------------
VARICODE_MAX_BITS = 10
PSK31_TRACEBACK_DEPTH = 32


def _bits_arg(bits, what="bits") -> np.ndarray:
    if not isinstance(bits, np.ndarray) or bits.dtype != np.uint8 or bits.ndim != 1:
        raise ValueError(f"{what}: expected a 1-D uint8 array")
    return np.ascontiguousarray(bits)


def _soft_arg(soft, batched) -> np.ndarray:
    if not isinstance(soft, np.ndarray) or soft.dtype != np.float32 or soft.ndim != (2 if batched else 1):
        raise ValueError(f"soft: expected a {'2' if batched else '1'}-D float32 array")
    if soft.shape[-1] % 2:
        raise ValueError("soft: an interleaved (re, im) pair per symbol, so an even length")
    return np.ascontiguousarray(soft)


def psk31_tables():
    """Host only: (varicode codewords uint16 (128,), MSB first; their lengths uint8 (128,);
    DQPSK_EXP float32 (4, 2)) as the library holds them (varicode.rs:27-156, psk31.rs:80-85)."""
    cw = np.zeros(128, np.uint16)
    ln = np.zeros(128, np.uint8)
    exp = np.zeros((4, 2), np.float32)
    _check(_L.orion_psk31_tables(cw.ctypes.data, ln.ctypes.data, exp.ctypes.data))
    return cw, ln, exp


def varicode_encode(byte: int):
    """varicode_encode (varicode.rs:163-169): (codeword, length); a byte >= 128 gives NUL's."""
    if not 0 <= int(byte) <= 255:
        raise ValueError("byte out of range")
    cw, ln = C.c_uint16(0), C.c_uint8(0)
    _check(_L.orion_varicode_encode(int(byte), C.byref(cw), C.byref(ln)))
    return cw.value, ln.value


def varicode_decode(bits: int, length: int):
    """varicode_decode (varicode.rs:176-183): the byte, or None for an unknown codeword."""
    if not (0 <= int(bits) <= 0xFFFF and 0 <= int(length) <= 255):
        raise ValueError("codeword out of range")
    r = _L.orion_varicode_decode(int(bits), int(length))
    return None if r < 0 else int(r)


class VaricodeEncoder:
    """VaricodeEncoder (varicode.rs:192-267; __init__.pyi:459-475), host only."""

    def __init__(self):
        self._h = _L.orion_varicode_encoder_new()
        if not self._h:
            raise OrionError(f"orion_sdr: {_err()}")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _L is not None:
            _L.orion_varicode_encoder_free(h)

    @staticmethod
    def _count(n) -> int:
        if int(n) < 0:
            raise ValueError("a bit count is not negative")
        return int(n)

    def push_preamble(self, n: int) -> None:
        rc = _L.orion_varicode_encoder_push_preamble(self._h, self._count(n))
        if rc == -3:
            raise ValueError(_err())
        _check(rc)

    def push_byte(self, b: int) -> None:
        if not 0 <= int(b) <= 255:
            raise ValueError("byte out of range")
        _check(_L.orion_varicode_encoder_push_byte(self._h, int(b)))

    def push_postamble(self, n: int) -> None:
        rc = _L.orion_varicode_encoder_push_postamble(self._h, self._count(n))
        if rc == -3:
            raise ValueError(_err())
        _check(rc)

    def drain_bits(self) -> np.ndarray:
        out = np.zeros(_L.orion_varicode_encoder_pending(self._h), np.uint8)
        n = C.c_size_t(0)
        _check(_L.orion_varicode_encoder_drain(self._h, out.ctypes.data, out.size, C.byref(n)))
        return out[:n.value]

    def is_empty(self) -> bool:
        return _L.orion_varicode_encoder_pending(self._h) == 0


class VaricodeDecoder:
    """VaricodeDecoder (varicode.rs:277-320; __init__.pyi:477-486), host only."""

    def __init__(self):
        self._h = _L.orion_varicode_decoder_new()
        if not self._h:
            raise OrionError(f"orion_sdr: {_err()}")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _L is not None:
            _L.orion_varicode_decoder_free(h)

    def push_bits(self, bits) -> None:
        bits = _bits_arg(bits)
        _check(_L.orion_varicode_decoder_push_bits(self._h, bits.ctypes.data, bits.size))

    def pop_bytes(self) -> bytes:
        out = np.zeros(_L.orion_varicode_decoder_pending(self._h), np.uint8)
        n = C.c_size_t(0)
        _check(_L.orion_varicode_decoder_pop_bytes(self._h, out.ctypes.data, out.size, C.byref(n)))
        return out[:n.value].tobytes()


def conv_encode(bits) -> np.ndarray:
    """conv_encode (psk31.rs:45-55): uint8 bits (n,) -> coded bits (2 n,), host only."""
    bits = _bits_arg(bits)
    out = np.zeros(2 * bits.size, np.uint8)
    _check(_L.orion_conv_encode(bits.ctypes.data, bits.size, out.ctypes.data))
    return out


def viterbi_decode(soft) -> np.ndarray:
    """viterbi_decode (psk31.rs:95-160) by the library's scalar decoder (host only; what the
    kernel is held to): float32 (2 n_syms,) -> uint8 bits (n_syms,)."""
    soft = _soft_arg(soft, False)
    out = np.zeros(soft.size // 2, np.uint8)
    _check(_L.orion_psk31_viterbi_host(soft.ctypes.data, out.size, out.ctypes.data))
    return out


def viterbi_decode_hard(coded) -> np.ndarray:
    """viterbi_decode_hard (psk31.rs:384-396): coded bits (2 n_syms,) -> bits (n_syms,), host only."""
    coded = _bits_arg(coded, "coded")
    if coded.size % 2:
        raise ValueError("coded: two bits per symbol, so an even length")
    out = np.zeros(coded.size // 2, np.uint8)
    _check(_L.orion_psk31_viterbi_hard_host(coded.ctypes.data, out.size, out.ctypes.data))
    return out


def psk31_viterbi_batch(soft, stream=None):
    """viterbi_decode of a batch of soft streams on the GPU in one launch (sixteen lanes per
    stream, four streams per wave): float32 (nstreams, 2 n_syms), a numpy array (-> numpy
    uint8 (nstreams, n_syms)) or a contiguous torch CUDA tensor (-> a torch uint8 tensor on
    its device, queued on torch's current stream or on stream)."""
    if _is_torch(soft):
        import torch

        if not soft.is_cuda or not soft.is_contiguous() or soft.dtype != torch.float32 or soft.dim() != 2:
            raise ValueError("psk31_viterbi_batch needs a contiguous 2-D float32 CUDA tensor")
        if soft.shape[1] % 2:
            raise ValueError("soft: an interleaved (re, im) pair per symbol, so an even length")
        ns, n = int(soft.shape[0]), int(soft.shape[1]) // 2
        bits = torch.empty((ns, n), dtype=torch.uint8, device=soft.device)
        wb = int(_L.orion_psk31_viterbi_work_bytes(ns, n))
        work = torch.empty(max(wb // 4, 1), dtype=torch.int32, device=soft.device)
        rc = _L.orion_psk31_viterbi_device(soft.data_ptr(), ns, n, bits.data_ptr(), work.data_ptr(), wb,
                                           SyncEngine._stream(soft, stream))
        if rc == -3:
            raise ValueError(_err())
        _check(rc)
        return bits
    soft = _soft_arg(soft, True)
    ns, n = soft.shape[0], soft.shape[1] // 2
    bits = np.zeros((ns, n), np.uint8)
    rc = _L.orion_psk31_viterbi(soft.ctypes.data, ns, n, bits.ctypes.data)
    if rc == -3:
        raise ValueError(_err())
    _check(rc)
    return bits


class StreamingViterbi:
    """StreamingViterbi (psk31.rs:257-377) on DQPSK_EXP, host only: feed(float32 (2 n,)) ->
    the bits that come out (none for a decoder's first 32 symbols), flush() -> the last 32."""

    def __init__(self):
        self._h = _L.orion_psk31_streaming_viterbi_new()
        if not self._h:
            raise OrionError(f"orion_sdr: {_err()}")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _L is not None:
            _L.orion_psk31_streaming_viterbi_free(h)

    def feed(self, soft) -> np.ndarray:
        soft = _soft_arg(soft, False)
        out = np.zeros(soft.size // 2, np.uint8)
        n = C.c_size_t(0)
        _check(_L.orion_psk31_streaming_viterbi_feed(self._h, soft.ctypes.data, out.size, out.ctypes.data, C.byref(n)))
        return out[:n.value]

    def flush(self) -> np.ndarray:
        out = np.zeros(PSK31_TRACEBACK_DEPTH, np.uint8)
        n = C.c_size_t(0)
        _check(_L.orion_psk31_streaming_viterbi_flush(self._h, out.ctypes.data, C.byref(n)))
        return out[:n.value]


# ---- PSK31 modulators and demodulators (src/modulate/psk31.rs, src/demodulate/psk31.rs) -------
PSK31_STREAM_DTYPE = np.dtype([("mode", np.uint32), ("channel", np.uint32), ("rf_hz", np.float32), ("gain", np.float32),
                               ("start", np.uint64), ("offset", np.uint32), ("out_cap", np.uint32)])
PSK31_REPORT_DTYPE = np.dtype([("in_read", np.uint64), ("out_written", np.uint64)])
_PSK31_MODES = {"bpsk": 0, "qpsk": 1, 0: 0, 1: 1}


def _arg_check(rc: int):
    if rc == -3:
        raise ValueError(_err())
    _check(rc)


def _iq_arg(iq, ndim=1) -> np.ndarray:
    if not isinstance(iq, np.ndarray) or iq.dtype != np.complex64 or iq.ndim != ndim:
        raise ValueError(f"iq: expected a {ndim}-D complex64 array")
    return np.ascontiguousarray(iq)


def psk31_sps(fs: float) -> int:
    """psk31_sps (modulate/psk31.rs:42-44): round(fs / 31.25) samples per symbol."""
    return int(_L.orion_psk31_sps(float(fs)))


def psk31_text_bits(text, preamble_bits: int = 32, postamble_bits: int = 32) -> np.ndarray:
    """The bits modulate_text sends (modulate/psk31.rs:146-159), host only."""
    text = bytes(text)
    if int(preamble_bits) < 0 or int(postamble_bits) < 0:
        raise ValueError("a bit count is not negative")
    n = C.c_size_t(0)
    rc = _L.orion_psk31_text_bits(text, len(text), int(preamble_bits), int(postamble_bits), None, 0, C.byref(n))
    if rc == -3 and n.value == 0:
        raise ValueError(_err())
    out = np.zeros(n.value, np.uint8)
    _arg_check(_L.orion_psk31_text_bits(text, len(text), int(preamble_bits), int(postamble_bits), out.ctypes.data, out.size,
                                        C.byref(n)))
    return out


class _Psk31Mod:
    """Bpsk31Mod / Qpsk31Mod (modulate/psk31.rs:110-216, :248-362; __init__.pyi:492-544): the
    library's host modulator in the reference's f32 operation order. The phasor (and
    QPSK31's coder register) is kept between calls; reset() returns to the start."""
    _mode = 0

    def __init__(self, fs: float, rf_hz: float, gain: float = 1.0):
        self._h = _L.orion_psk31_mod_new(self._mode, float(fs), float(rf_hz), float(gain))
        if not self._h:
            raise ValueError(f"orion_sdr: {_err()}")
        self.sps = psk31_sps(fs)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _L is not None:
            _L.orion_psk31_mod_free(h)

    def set_gain(self, g: float) -> None:
        _check(_L.orion_psk31_mod_set_gain(self._h, float(g)))

    def reset(self) -> None:
        _check(_L.orion_psk31_mod_reset(self._h))

    def modulate_bits(self, bits, device=False, stream=None):
        """bits uint8 (n,) -> iq complex64 (n * sps,): a numpy array from the host modulator, or
        with device=True a torch tensor on the current device from the kernel (the same bytes;
        the state advances either way)."""
        bits = _bits_arg(bits)
        if device:
            import torch

            out = torch.empty(bits.size * self.sps, dtype=torch.complex64, device="cuda")
            _arg_check(_L.orion_psk31_mod_modulate_bits_device(self._h, bits.ctypes.data, bits.size, out.data_ptr(),
                                                               SyncEngine._stream(out, stream)))
            return out
        out = np.zeros(bits.size * self.sps, np.complex64)
        _check(_L.orion_psk31_mod_modulate_bits(self._h, bits.ctypes.data, bits.size, out.ctypes.data))
        return out

    def modulate_batch(self, bits, device=False, stream=None):
        """bits uint8 (nstreams, n) -> iq complex64 (nstreams, n * sps) by one kernel launch,
        every stream from a fresh modulator of these parameters (this one's state is not
        touched): numpy, or with device=True a torch tensor."""
        if not isinstance(bits, np.ndarray) or bits.dtype != np.uint8 or bits.ndim != 2:
            raise ValueError("bits: expected a 2-D uint8 array")
        bits = np.ascontiguousarray(bits)
        ns, n = bits.shape
        if device:
            import torch

            out = torch.empty((ns, n * self.sps), dtype=torch.complex64, device="cuda")
            _arg_check(_L.orion_psk31_mod_modulate_batch_device(self._h, bits.ctypes.data, ns, n, out.data_ptr(),
                                                                SyncEngine._stream(out, stream)))
            return out
        out = np.zeros((ns, n * self.sps), np.complex64)
        _arg_check(_L.orion_psk31_mod_modulate_batch(self._h, bits.ctypes.data, ns, n, out.ctypes.data))
        return out

    def modulate_text(self, text, preamble_bits: int = 32, postamble_bits: int = 32, device=False):
        return self.modulate_bits(psk31_text_bits(text, preamble_bits, postamble_bits), device=device)

    def process(self, bits, out_cap: int):
        """Block::process (:199-215): -> (iq written, bits read)."""
        bits = _bits_arg(bits)
        out = np.zeros(int(out_cap), np.complex64)
        wr = WorkReport()
        _check(_L.orion_psk31_mod_process(self._h, bits.ctypes.data, bits.size, out.ctypes.data, out.size, C.byref(wr)))
        return out[:wr.out_written], int(wr.in_read)


class Bpsk31Mod(_Psk31Mod):
    _mode = 0


class Qpsk31Mod(_Psk31Mod):
    _mode = 1


class Psk31DemodBank:
    """nstreams independent BPSK31 / QPSK31 demodulators over nch channels, advanced by one
    kernel launch per call (one lane per stream). records: a PSK31_STREAM_DTYPE array (mode 0
    BPSK / 1 QPSK, channel, rf_hz, gain, start sample, offset as new_with_offset, out_cap soft
    values per call). process(iq (nch, n) complex64) -> (soft float32 (nstreams, out_stride),
    bits uint8 the same shape (soft >= 0 for BPSK31 streams, zeros for QPSK31 streams, whose
    decisions are the Viterbi decoder's), reports PSK31_REPORT_DTYPE (nstreams,)); row k
    holds out_written[k] values. numpy in, numpy out; a torch CUDA tensor in, torch tensors
    out (reports as an int64 (nstreams, 2) tensor) on torch's current stream. State is carried
    between calls: chunked calls give one call's bytes."""

    def __init__(self, fs: float, records, nch: int = 1):
        if not isinstance(records, np.ndarray) or records.dtype != PSK31_STREAM_DTYPE or records.ndim != 1:
            raise ValueError("records: expected a 1-D PSK31_STREAM_DTYPE array")
        records = np.ascontiguousarray(records)
        self._h = _L.orion_psk31_demod_bank_new(float(fs), records.ctypes.data, records.size, int(nch))
        if not self._h:
            raise ValueError(f"orion_sdr: {_err()}")
        self.nstreams, self.nch = int(records.size), int(nch)
        self.out_stride = max(int(records["out_cap"].max()), 1)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _L is not None:
            _L.orion_psk31_demod_bank_free(h)

    def reset(self) -> None:
        _check(_L.orion_psk31_demod_bank_reset(self._h))

    def set_gain(self, index: int, gain: float) -> None:
        _arg_check(_L.orion_psk31_demod_bank_set_gain(self._h, int(index), float(gain)))

    def process(self, iq, want_bits=True, stream=None):
        if _is_torch(iq):
            import torch

            if not iq.is_cuda or not iq.is_contiguous() or iq.dtype != torch.complex64 or iq.dim() != 2:
                raise ValueError("Psk31DemodBank.process needs a contiguous (nch, n) complex64 CUDA tensor")
            soft = torch.zeros((self.nstreams, self.out_stride), dtype=torch.float32, device=iq.device)
            bits = torch.zeros((self.nstreams, self.out_stride), dtype=torch.uint8, device=iq.device) if want_bits else None
            rep = torch.zeros((self.nstreams, 2), dtype=torch.int64, device=iq.device)
            _arg_check(_L.orion_psk31_demod_bank_process_device(
                self._h, iq.data_ptr(), int(iq.shape[0]), int(iq.shape[1]), soft.data_ptr(), self.out_stride,
                bits.data_ptr() if want_bits else None, rep.data_ptr(), SyncEngine._stream(iq, stream)))
            return soft, bits, rep
        return self.process_host(iq, want_bits)

    def process_host(self, iq, want_bits=True):
        iq = _iq_arg(iq, 2)
        soft = np.zeros((self.nstreams, self.out_stride), np.float32)
        bits = np.zeros((self.nstreams, self.out_stride), np.uint8) if want_bits else None
        rep = np.zeros(self.nstreams, PSK31_REPORT_DTYPE)
        _arg_check(_L.orion_psk31_demod_bank_process(self._h, iq.ctypes.data, iq.shape[0], iq.shape[1], soft.ctypes.data,
                                                     self.out_stride, bits.ctypes.data if want_bits else None,
                                                     rep.ctypes.data))
        return soft, bits, rep


class _Psk31Demod:
    """Bpsk31Demod / Qpsk31Demod (demodulate/psk31.rs:83-220, :271-397; __init__.pyi:510-561).
    process runs on the GPU, as a bank of one stream (one lane: the chain is serial in time, so
    a single stream is slower there than on the host; the bank is for many). process_host is
    the library's scalar demodulator, the reference's arithmetic with glibc's sine and cosine;
    the two keep separate state."""
    _mode = 0

    def __init__(self, fs: float, rf_hz: float, gain: float = 1.0, offset: int = 0):
        if int(offset) < 0:
            raise ValueError("offset is not negative")
        self._fs, self._rf, self._gain, self._offset = float(fs), float(rf_hz), float(gain), int(offset)
        self._h = _L.orion_psk31_demod_new(self._mode, self._fs, self._rf, self._gain, self._offset)
        if not self._h:
            raise ValueError(f"orion_sdr: {_err()}")
        self.sps = psk31_sps(fs)
        self._bank = None
        self._bank_cap = 0
        self._soft = []

    @classmethod
    def new_with_offset(cls, fs: float, rf_hz: float, gain: float, offset: int):
        return cls(fs, rf_hz, gain, offset)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _L is not None:
            _L.orion_psk31_demod_free(h)

    def set_gain(self, g: float) -> None:
        self._gain = float(g)
        _check(_L.orion_psk31_demod_set_gain(self._h, self._gain))
        if self._bank is not None:
            self._bank.set_gain(0, self._gain)

    def reset(self) -> None:
        _check(_L.orion_psk31_demod_reset(self._h))
        if self._bank is not None:
            self._bank.reset()
        self._soft = []

    def _cap(self, n: int) -> int:
        return (n // self.sps + 2) * (2 if self._mode else 1)

    _BANK_CAP = 4096  # soft values per bank call; longer inputs go through in slices

    def process(self, iq) -> np.ndarray:
        iq = _iq_arg(iq)
        if self._bank is None:
            rec = np.zeros(1, PSK31_STREAM_DTYPE)
            rec[0] = (self._mode, 0, self._rf, self._gain, 0, self._offset, self._BANK_CAP)
            self._bank = Psk31DemodBank(self._fs, rec, 1)
        step = (self._BANK_CAP // 2 - 2) * self.sps  # a slice never fills the capacity, so none is cut short
        parts = []
        for at in range(0, iq.size, step):
            soft, _, rep = self._bank.process_host(iq[at:at + step].reshape(1, -1), want_bits=False)
            parts.append(soft[0, :int(rep["out_written"][0])].copy())
        out = np.concatenate(parts) if parts else np.zeros(0, np.float32)
        self._soft.append(out)
        return out

    def process_host(self, iq, out_cap=None):
        """-> (soft, in_read) by the scalar host demodulator, with the reference's loop
        conditions for an output of out_cap values (default: room for every symbol)."""
        iq = _iq_arg(iq)
        out = np.zeros(self._cap(iq.size) if out_cap is None else int(out_cap), np.float32)
        wr = WorkReport()
        _check(_L.orion_psk31_demod_process(self._h, iq.ctypes.data, iq.size, out.ctypes.data, out.size, C.byref(wr)))
        return out[:wr.out_written].copy(), int(wr.in_read)


class Bpsk31Demod(_Psk31Demod):
    _mode = 0


class Qpsk31Demod(_Psk31Demod):
    _mode = 1

    def flush(self) -> np.ndarray:
        """Qpsk31Decider::flush (demodulate/psk31.rs:422-428): the Viterbi decode (on the GPU)
        of every soft pair process() has returned since the last flush."""
        soft = np.concatenate(self._soft) if self._soft else np.zeros(0, np.float32)
        self._soft = []
        if soft.size == 0:
            return np.zeros(0, np.uint8)
        return psk31_viterbi_batch(soft.reshape(1, -1))[0]


class Bpsk31Decider:
    """Bpsk31Decider (demodulate/psk31.rs:228-261): bit = soft >= 0, host only."""

    def process(self, soft) -> np.ndarray:
        if not isinstance(soft, np.ndarray) or soft.dtype != np.float32 or soft.ndim != 1:
            raise ValueError("soft: expected a 1-D float32 array")
        soft = np.ascontiguousarray(soft)
        out = np.zeros(soft.size, np.uint8)
        _check(_L.orion_bpsk31_decide(soft.ctypes.data, soft.size, out.ctypes.data))
        return out


PSK31_SIGNAL_DTYPE = np.dtype([("channel", np.uint32), ("mode", np.uint32), ("offset", np.int64), ("rf_hz", np.float32),
                               ("gain", np.float32), ("n_bits", np.uint64)])


def psk31_rotator_q64(freq_hz: float, fs: float) -> int:
    """The angle of Rotator(freq_hz, fs)'s f32 step phasor as a Q0.64 turn count (host only):
    what psk31_synth's RF stage is the closed form of."""
    return int(_L.orion_psk31_rotator_q64(float(freq_hz), float(fs)))


def psk31_synth(signals, bits, n, nch=1, fs=8000.0, out=None, accumulate=False, device=False, stream=None):
    """Many PSK31 signals summed into many channels in one launch: signals a
    PSK31_SIGNAL_DTYPE array (channel, mode 0 BPSK / 1 QPSK, offset, rf_hz, gain; n_bits is
    filled in here), bits a list of uint8 arrays, one per signal -> iq complex64 (nch, n).
    out + accumulate=True adds to an existing buffer. numpy, or with device=True a torch
    tensor (out must then be a CUDA tensor if given)."""
    if not isinstance(signals, np.ndarray) or signals.dtype != PSK31_SIGNAL_DTYPE or signals.ndim != 1:
        raise ValueError("signals: expected a 1-D PSK31_SIGNAL_DTYPE array")
    if len(bits) != signals.size:
        raise ValueError("bits: one uint8 array per signal")
    rows = [_bits_arg(b) for b in bits]
    sig = np.ascontiguousarray(signals).copy()
    sig["n_bits"] = [r.size for r in rows]
    allbits = np.ascontiguousarray(np.concatenate(rows)) if rows and sum(r.size for r in rows) else np.zeros(1, np.uint8)
    n, nch = int(n), int(nch)
    if n < 0 or nch < 1:
        raise ValueError("n >= 0 and nch >= 1")
    if device or (out is not None and _is_torch(out)):
        import torch

        if out is None:
            out = torch.zeros((nch, n), dtype=torch.complex64, device="cuda")
        elif not (_is_torch(out) and out.is_cuda and out.is_contiguous() and out.dtype == torch.complex64
                  and tuple(out.shape) == (nch, n)):
            raise ValueError("out: a contiguous (nch, n) complex64 CUDA tensor")
        _arg_check(_L.orion_psk31_synth_device(float(fs), sig.ctypes.data, allbits.ctypes.data, sig.size, nch, n,
                                               1 if accumulate else 0, out.data_ptr(), SyncEngine._stream(out, stream)))
        return out
    if out is None:
        out = np.zeros((nch, n), np.complex64)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.complex64 and out.shape == (nch, n) and out.flags.c_contiguous):
        raise ValueError("out: a C-contiguous (nch, n) complex64 array")
    _arg_check(_L.orion_psk31_synth(float(fs), sig.ctypes.data, allbits.ctypes.data, sig.size, nch, n, 1 if accumulate else 0,
                                    out.ctypes.data))
    return out


# ---- PSK31 carrier search, sync and the band browser (src/sync/psk31_sync.rs) ----------------
PSK31_BAUD = 31.25


def psk31_find_carriers(wf, min_carrier_syms: int = 8, peak_margin_db: float = 6.0, max_cand: int = 10):
    """The search of psk31_sync (psk31_sync.rs:82-203) over a log waterfall, on the host: wf
    float32 (num_syms, num_bins) -> a CANDIDATE_DTYPE array, score descending (equal scores
    by freq_bin, then time_sym), or (nch, num_syms, num_bins) -> a list of them."""
    if not isinstance(wf, np.ndarray) or wf.dtype != np.float32 or wf.ndim not in (2, 3):
        raise ValueError("wf: expected a 2-D or 3-D float32 array")
    if int(max_cand) < 1:
        raise ValueError("max_cand == 0")
    if int(min_carrier_syms) < 0:
        raise ValueError("min_carrier_syms is not negative")
    w3 = np.ascontiguousarray(wf if wf.ndim == 3 else wf[None])
    nch = w3.shape[0]
    cand = np.zeros((nch, int(max_cand)), CANDIDATE_DTYPE)
    count = np.zeros(nch, np.uint32)
    _arg_check(_L.orion_psk31_find_carriers_host(w3.ctypes.data, nch, w3.shape[1], w3.shape[2], int(min_carrier_syms),
                                                 float(peak_margin_db), int(max_cand), cand.ctypes.data,
                                                 count.ctypes.data))
    out = [cand[ch, :count[ch]].copy() for ch in range(nch)]
    return out if wf.ndim == 3 else out[0]


def psk31_find_carriers_device(wf, min_carrier_syms: int = 8, peak_margin_db: float = 6.0, max_cand: int = 10,
                                stream=None):
    """The same search by the device kernels (orion_psk31_find_carriers / _device): wf float32
    (num_syms, num_bins) or (nch, num_syms, num_bins), a numpy array or a contiguous torch CUDA
    tensor. -> as psk31_find_carriers (numpy either way); equal to it, order and scores
    included."""
    tw = _is_torch(wf)
    if tw:
        import torch

        if not wf.is_cuda or not wf.is_contiguous() or wf.dtype != torch.float32 or wf.dim() not in (2, 3):
            raise ValueError("wf: expected a contiguous 2-D or 3-D float32 CUDA tensor")
    elif not isinstance(wf, np.ndarray) or wf.dtype != np.float32 or wf.ndim not in (2, 3):
        raise ValueError("wf: expected a 2-D or 3-D float32 array")
    if int(max_cand) < 1:
        raise ValueError("max_cand == 0")
    if int(min_carrier_syms) < 0:
        raise ValueError("min_carrier_syms is not negative")
    three = len(wf.shape) == 3
    nch, num_syms, num_bins = (int(v) for v in (wf.shape if three else (1,) + tuple(wf.shape)))
    eng = _sync_engine()
    if tw:
        import torch

        cand = torch.zeros((nch, int(max_cand), 3), dtype=torch.int32, device=wf.device)
        count = torch.zeros(nch, dtype=torch.int32, device=wf.device)
        _arg_check(_L.orion_psk31_find_carriers_device(eng._h, wf.data_ptr(), nch, num_syms, num_bins,
                                                       int(min_carrier_syms), float(peak_margin_db), int(max_cand),
                                                       cand.data_ptr(), count.data_ptr(), SyncEngine._stream(wf, stream)))
        hc = cand.cpu().numpy().view(CANDIDATE_DTYPE)[..., 0]
        hn = count.cpu().numpy().view(np.uint32)
    else:
        w3 = np.ascontiguousarray(wf)
        hc = np.zeros((nch, int(max_cand)), CANDIDATE_DTYPE)
        hn = np.zeros(nch, np.uint32)
        _arg_check(_L.orion_psk31_find_carriers(eng._h, w3.ctypes.data, nch, num_syms, num_bins, int(min_carrier_syms),
                                                float(peak_margin_db), int(max_cand), hc.ctypes.data, hn.ctypes.data))
    out = [hc[ch, :hn[ch]].copy() for ch in range(nch)]
    return out if three else out[0]


def psk31_sync_batch(iq, fs, base_hz, max_hz, min_carrier_syms=8, peak_margin_db=6.0, n_bits=1024, max_cand=10,
                     stream=None):
    """psk31_sync (psk31_sync.rs:50-205) for every row of iq (nch, n) complex64, one device
    call with no trip to the host between its stages (orion_psk31_sync / _device): the
    waterfall (one bin per 31.25 Hz), the carrier search, the candidates' bank records
    written on the device, and every kept candidate's soft bits from one launch of the
    demodulator bank (record_candidate, :209-239: a BPSK31 stream at base_hz + freq_bin *
    31.25 from sample time_sym * sps, gain 1, capacity n_bits + 2, the first min(out_written,
    n_bits) values). iq: a numpy array (uploaded once) or a contiguous torch CUDA tensor (it
    stays where it is). -> per channel a list of dicts time_sym, freq_bin, carrier_hz, score,
    soft_bits (numpy)."""
    ti = _is_torch(iq)
    if ti:
        import torch

        if not iq.is_cuda or not iq.is_contiguous() or iq.dtype != torch.complex64 or iq.dim() != 2:
            raise ValueError("psk31_sync_batch needs a contiguous (nch, n) complex64 CUDA tensor")
    else:
        iq = _iq_arg(iq, 2)
    if int(max_cand) < 1:
        raise ValueError("max_cand == 0")
    if int(n_bits) < 0 or int(n_bits) > (1 << 30) - 2:
        raise ValueError("n_bits out of range")
    if int(min_carrier_syms) < 0:
        raise ValueError("min_carrier_syms is not negative")
    nch, n = int(iq.shape[0]), int(iq.shape[1])
    sps = psk31_sps(fs)
    if sps == 0 or n // sps == 0:
        return [[] for _ in range(nch)]
    mc, nb = int(max_cand), int(n_bits)
    args = (nch, n, float(fs), float(base_hz), float(max_hz), int(min_carrier_syms), float(peak_margin_db), nb, mc)
    eng = _sync_engine()
    if ti:
        import torch

        cand = torch.zeros((nch, mc, 3), dtype=torch.int32, device=iq.device)
        count = torch.zeros(nch, dtype=torch.int32, device=iq.device)
        soft = torch.zeros((nch, mc, nb + 2), dtype=torch.float32, device=iq.device)
        rep = torch.zeros((nch, mc, 2), dtype=torch.int64, device=iq.device)
        _arg_check(_L.orion_psk31_sync_device(eng._h, iq.data_ptr(), *args, cand.data_ptr(), count.data_ptr(),
                                              soft.data_ptr(), rep.data_ptr(), SyncEngine._stream(iq, stream)))
        cand = cand.cpu().numpy().view(CANDIDATE_DTYPE)[..., 0]
        count = count.cpu().numpy().view(np.uint32)
        soft, rep = soft.cpu().numpy(), rep.cpu().numpy()
    else:
        cand = np.zeros((nch, mc), CANDIDATE_DTYPE)
        count = np.zeros(nch, np.uint32)
        soft = np.zeros((nch, mc, nb + 2), np.float32)
        rep = np.zeros((nch, mc, 2), np.int64)
        _arg_check(_L.orion_psk31_sync(eng._h, iq.ctypes.data, *args, cand.ctypes.data, count.ctypes.data,
                                       soft.ctypes.data, rep.ctypes.data))
    out = []
    for ch in range(nch):
        row = []
        for k in range(int(count[ch])):
            c = cand[ch, k]
            carrier = float(np.float32(base_hz) + np.float32(c["freq_bin"]) * np.float32(PSK31_BAUD))
            keep = min(int(rep[ch, k, 1]), nb)
            row.append({"time_sym": int(c["time_sym"]), "freq_bin": int(c["freq_bin"]), "carrier_hz": carrier,
                        "score": float(c["score"]), "soft_bits": soft[ch, k, :keep].copy()})
        out.append(row)
    return out


def psk31_sync(iq, fs, base_hz, max_hz, min_carrier_syms=8, peak_margin_db=6.0, n_bits=1024, max_cand=10):
    """psk31_sync (__init__.pyi:591-613) of one buffer: a list of candidate dicts."""
    iq = _iq_arg(iq)
    return psk31_sync_batch(iq.reshape(1, -1), fs, base_hz, max_hz, min_carrier_syms, peak_margin_db, n_bits, max_cand)[0]


def best_psk31_sync(candidates, carrier_hz, baud=PSK31_BAUD):
    """best_psk31_sync (__init__.pyi:615-625): of the candidates within 2 * baud of
    carrier_hz the one with the highest score (the first of equals), or None."""
    best = None
    for c in candidates:
        if abs(c["carrier_hz"] - carrier_hz) <= 2.0 * baud and (best is None or c["score"] > best["score"]):
            best = c
    return best


def _varicode_text(bits) -> str:
    d = VaricodeDecoder()
    d.push_bits(np.ascontiguousarray(bits, np.uint8))
    d.push_bits(np.zeros(2, np.uint8))
    return "".join(chr(b) for b in d.pop_bytes() if 0x20 <= b < 0x7F)


def psk31_decode_batch(iq, fs, base_hz, max_hz, min_carrier_syms=8, peak_margin_db=6.0, n_bits=1024, max_cand=10):
    """The band browser: psk31_sync_batch, then each candidate's hard bits (soft >= 0) through
    Varicode (printable ASCII kept, as Psk31Stream does). -> per channel a list of dicts
    carrier_hz, score, time_sym, text."""
    out = []
    for cands in psk31_sync_batch(iq, fs, base_hz, max_hz, min_carrier_syms, peak_margin_db, n_bits, max_cand):
        out.append([{"carrier_hz": c["carrier_hz"], "score": c["score"], "time_sym": c["time_sym"],
                     "text": _varicode_text(c["soft_bits"] >= 0)} for c in cands])
    return out


def psk31_decode(iq, fs, base_hz, max_hz, min_carrier_syms=8, peak_margin_db=6.0, n_bits=1024, max_cand=10):
    iq = _iq_arg(iq)
    return psk31_decode_batch(iq.reshape(1, -1), fs, base_hz, max_hz, min_carrier_syms, peak_margin_db, n_bits, max_cand)[0]


class Psk31Stream:
    """Psk31Stream (codec/psk31.rs:416-572; __init__.pyi:567-585): feed(iq) -> newly decoded
    printable text, flush() -> the rest. The demodulator runs on the device (a bank of one
    stream; device=False: the library's scalar host demodulator), the decider or the
    streaming Viterbi decoder and Varicode on the host. QPSK31 symbols with d_re^2 + d_im^2 <
    0.01 are skipped (:519)."""

    def __init__(self, mode: str, fs: float, carrier_hz: float, gain: float = 1.0, device: bool = True):
        if mode not in ("bpsk", "qpsk"):
            raise ValueError("mode: 'bpsk' or 'qpsk'")
        self._qpsk = mode == "qpsk"
        self._demod = (Qpsk31Demod if self._qpsk else Bpsk31Demod)(fs, carrier_hz, gain)
        self._device = bool(device)
        self._vit = StreamingViterbi() if self._qpsk else None
        self._vdec = VaricodeDecoder()
        self.fed_up_to = 0

    def set_fed_up_to(self, v: int) -> None:
        self.fed_up_to = int(v)

    def _text(self, bits) -> str:
        self._vdec.push_bits(np.ascontiguousarray(bits, np.uint8))
        return "".join(chr(b) for b in self._vdec.pop_bytes() if 0x20 <= b < 0x7F)

    def feed(self, iq) -> str:
        iq = _iq_arg(iq)
        if iq.size == 0:
            return ""
        soft = self._demod.process(iq) if self._device else self._demod.process_host(iq)[0]
        self._demod._soft = []  # the stream decodes as it goes; nothing is kept for flush()
        if not self._qpsk:
            return self._text(soft >= 0)
        pairs = soft.reshape(-1, 2)
        re, im = pairs[:, 0], pairs[:, 1]
        keep = ~(re * re + im * im < np.float32(0.01))
        return self._text(self._vit.feed(np.ascontiguousarray(pairs[keep].reshape(-1))))

    def flush(self) -> str:
        text = self._text(self._vit.flush()) if self._qpsk else ""
        return text + self._text(np.zeros(2, np.uint8))


def pinned_empty(shape, dtype) -> np.ndarray:
    """A numpy array in pinned host memory (orion_host_alloc): the host-buffer path
    (orion_block_process) DMAs it without staging copies. Freed with the array."""
    import weakref

    dt = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dt.itemsize
    p = _L.orion_host_alloc(max(1, nbytes))
    if not p:
        raise OrionError(f"orion_sdr: pinned allocation failed: {_err()}")
    buf = (C.c_char * max(1, nbytes)).from_address(p)
    weakref.finalize(buf, _L.orion_host_free, C.c_void_p(p))
    return np.frombuffer(buf, dt, count=int(np.prod(shape))).reshape(shape)


def device_count() -> int:
    return _L.orion_device_count()


def version() -> str:
    return _L.orion_version().decode()


# ---- the OFDM symbol layer (src/multicarrier, modulate/ofdm.rs, demodulate/ofdm.rs; src/python/ofdm.rs) ----
def _ofdm_sigs():
    vp, sz, f, i = C.c_void_p, C.c_size_t, C.c_float, C.c_int
    wr = C.POINTER(WorkReport)
    sig = {
        "orion_ofdm_config_new": (vp, [sz, sz, vp, sz, vp, vp, sz, f, f, f, i]),
        "orion_ofdm_config_free": (None, [vp]),
        "orion_ofdm_config_contiguous_data": (i, [vp, sz, i]),
        "orion_ofdm_config_set_rx_window_backoff": (i, [vp, sz]),
        "orion_ofdm_config_set_symbol_window": (i, [vp, sz]),
        "orion_ofdm_config_validate": (i, [vp, C.c_longlong, C.POINTER(C.c_int32)]),
        "orion_ofdm_config_info": (i, [vp, C.POINTER(sz)]),
        "orion_ofdm_config_data_carriers": (i, [vp, vp, sz]),
        "orion_ofdm_config_occupied_bins": (i, [vp, vp, sz, C.POINTER(sz)]),
        "orion_ofdm_config_grid": (i, [vp, vp, vp]),
        "orion_ofdm_max_pilot_safe_backoff": (sz, [sz, sz]),
        "orion_ofdm_tables": (i, [i, vp, vp, sz, vp, vp, sz, sz, vp]),
        "orion_ofdm_map_host": (i, [i, vp, sz, vp]), "orion_ofdm_decide_host": (i, [i, vp, sz, vp]),
        "orion_ofdm_llr_host": (i, [i, vp, sz, vp]), "orion_fft_host": (i, [sz, i, vp, sz, vp]),
        "orion_ofdm_window_host": (i, [sz, sz, vp, sz]), "orion_ofdm_rotator_host": (i, [f, f, sz, vp]),
        "orion_ofdm_evm_db_host": (i, [i, vp, sz, vp, sz, sz, C.POINTER(f), C.POINTER(i)]),
        "orion_ofdm_equalizer_weight_host": (i, [vp, sz, vp]),
        "orion_ofdm_interpolate_host": (i, [vp, vp, sz, vp, sz, vp]),
        "orion_fft_new": (vp, [sz]), "orion_ifft_new": (vp, [sz]), "orion_fft_free": (None, [vp]),
        "orion_fft_process": (i, [vp, vp, sz, vp, sz, wr]),
        "orion_fft_batch": (i, [vp, vp, sz, vp, sz, sz, vp]),
        "orion_ofdm_mod_new": (vp, [vp]), "orion_ofdm_demod_new": (vp, [vp, i]),
        "orion_ofdm_decider_new": (vp, [vp]), "orion_ofdm_soft_demod_new": (vp, [vp]),
        "orion_ofdm_equalizer_new": (vp, [vp, i]), "orion_ofdm_free": (None, [vp]),
        "orion_ofdm_set_gain": (i, [vp, f]), "orion_ofdm_reset": (i, [vp]),
        "orion_ofdm_estimate_channel": (i, [vp, vp, sz]),
        "orion_ofdm_process": (i, [vp, vp, sz, vp, sz, wr]),
        "orion_ofdm_mod_device": (i, [vp, vp, sz, sz, vp, vp]),
        "orion_ofdm_demod_device": (i, [vp, vp, sz, sz, vp, vp, vp, vp]),
        "orion_ofdm_decider_device": (i, [vp, vp, sz, sz, vp, vp]),
        "orion_ofdm_soft_demod_device": (i, [vp, vp, sz, sz, vp, vp]),
        "orion_ofdm_equalizer_device": (i, [vp, vp, sz, sz, vp, vp]),
        "orion_ofdm_mod_host": (i, [vp, vp, sz, vp, sz, wr]), "orion_ofdm_demod_host": (i, [vp, vp, sz, vp, sz, wr]),
        "orion_ofdm_equalize_host": (i, [vp, vp, sz, vp, sz, wr]),
        "orion_ofdm_set_pilot_bins_host": (i, [vp, vp, vp, sz, vp, sz]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(_L, name)
        fn.restype = res
        fn.argtypes = args


_ofdm_sigs()

OFDM_CONSTELLATIONS = {"bpsk": 0, "qpsk": 1, "qam16": 2, "qam64": 3, "qam256": 4}  # src/python/ofdm.rs:29-41
OFDM_PLAN_ERRORS = {1: "out_of_range", 2: "overlap", 3: "empty_data_set", 4: "in_guard_band"}  # config.rs:17-26
_OFDM_EQ = {None: -1, "training_symbol": 0, "pilot_interp": 1}  # src/python/ofdm.rs:532-541


def _ofdm_arr(x, dtype, name):
    """1-D contiguous input of exactly this dtype (src/python/ofdm.rs takes PyReadonlyArray1 slices)."""
    if not isinstance(x, np.ndarray) or x.dtype != dtype or x.ndim != 1 or not x.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{name}: expected a 1-D contiguous {np.dtype(dtype).name} array")
    return x


def _ofdm_order(constellation) -> int:
    if constellation not in OFDM_CONSTELLATIONS:
        raise ValueError(f"unknown constellation {constellation!r} (expected one of {sorted(OFDM_CONSTELLATIONS)})")
    return OFDM_CONSTELLATIONS[constellation]


def ofdm_max_pilot_safe_backoff(n_fft: int, pilot_spacing: int) -> int:
    """SymbolFft::max_pilot_safe_backoff (symbol_fft.rs:90-92)."""
    return int(_L.orion_ofdm_max_pilot_safe_backoff(int(n_fft), int(pilot_spacing)))


def ofdm_tables(constellation="qam16", n_fft=0, symbol_len=0, roll_off=0):
    """(axis float32 (16,), thresholds float32 (15,), training complex64 (n_fft,), twiddles
    complex64 (n_fft // 2,), ramp float32) as the library holds them (modulate/qam.rs:27-57,
    demodulate/qam.rs:28-41, sync/ofdm_sync.rs:270-352, symbol_window.rs:47-59), host only."""
    axis, thr = np.zeros(16, np.float32), np.zeros(15, np.float32)
    tr, tw = np.zeros(int(n_fft), np.complex64), np.zeros(int(n_fft) // 2, np.complex64)
    ramp = np.zeros(min(int(roll_off), int(symbol_len) // 2), np.float32)
    _arg_check(_L.orion_ofdm_tables(_ofdm_order(constellation), axis.ctypes.data, thr.ctypes.data, int(n_fft),
                                    tr.ctypes.data if n_fft else None, tw.ctypes.data if n_fft else None,
                                    int(symbol_len), int(roll_off), ramp.ctypes.data if ramp.size else None))
    return axis, thr, tr, tw, ramp


def ofdm_map(constellation, bits) -> np.ndarray:
    """The symbol mapper of an order on the host: uint8 bits -> complex64 symbols."""
    bits = _ofdm_arr(bits, np.uint8, "bits")
    order = _ofdm_order(constellation)
    n = bits.size // (1, 2, 4, 6, 8)[order]
    out = np.zeros(n, np.complex64)
    _arg_check(_L.orion_ofdm_map_host(order, bits.ctypes.data, n, out.ctypes.data))
    return out


def ofdm_decide(constellation, syms) -> np.ndarray:
    """The hard decider of an order on the host: complex64 symbols -> uint8 bits."""
    syms = _ofdm_arr(syms, np.complex64, "syms")
    order = _ofdm_order(constellation)
    out = np.zeros(syms.size * (1, 2, 4, 6, 8)[order], np.uint8)
    _arg_check(_L.orion_ofdm_decide_host(order, syms.ctypes.data, syms.size, out.ctypes.data))
    return out


def ofdm_llr(constellation, syms) -> np.ndarray:
    """The max-log LLRs of an order on the host (positive = 0): complex64 symbols -> float32."""
    syms = _ofdm_arr(syms, np.complex64, "syms")
    order = _ofdm_order(constellation)
    out = np.zeros(syms.size * (1, 2, 4, 6, 8)[order], np.float32)
    _arg_check(_L.orion_ofdm_llr_host(order, syms.ctypes.data, syms.size, out.ctypes.data))
    return out


def fft_host(x, n_fft: int, inverse: bool = False) -> np.ndarray:
    """The library's scalar radix-2 transform of every whole n_fft-point symbol of x (host only)."""
    x = _ofdm_arr(x, np.complex64, "x")
    n_fft = int(n_fft)
    k = x.size // n_fft if n_fft > 0 else 0
    out = np.zeros(k * n_fft, np.complex64)
    _arg_check(_L.orion_fft_host(n_fft, int(bool(inverse)), x.ctypes.data, k, out.ctypes.data))
    return out


def ofdm_window(iq, symbol_len: int, roll_off: int) -> np.ndarray:
    """SymbolWindow (symbol_window.rs:80-98) over every whole symbol of iq, host only."""
    iq = _ofdm_arr(iq, np.complex64, "iq").copy()
    if symbol_len > 0:
        _arg_check(_L.orion_ofdm_window_host(int(symbol_len), int(roll_off), iq.ctypes.data, iq.size // int(symbol_len)))
    return iq


def ofdm_rotator(freq_hz: float, fs: float, n: int) -> np.ndarray:
    """Rotator(freq_hz, fs).next() n times from a fresh oscillator (dsp/rotator.rs:16-61), host only."""
    out = np.zeros(int(n), np.complex64)
    _check(_L.orion_ofdm_rotator_host(float(freq_hz), float(fs), out.size, out.ctypes.data))
    return out


def ofdm_equalizer_weight(h) -> np.ndarray:
    """equalizer_weight (demodulate/ofdm.rs:495-502) of each estimate, host only."""
    h = _ofdm_arr(h, np.complex64, "h")
    out = np.zeros(h.size, np.complex64)
    _check(_L.orion_ofdm_equalizer_weight_host(h.ctypes.data, h.size, out.ctypes.data))
    return out


def ofdm_interpolate(pilot_bins, ratios, bins) -> np.ndarray:
    """interpolate_at (demodulate/ofdm.rs:514-537) over bin-sorted pilot ratios, host only."""
    pb = np.ascontiguousarray(pilot_bins, np.uint32)
    r = _ofdm_arr(ratios, np.complex64, "ratios")
    b = np.ascontiguousarray(bins, np.uint32)
    if pb.size != r.size:
        raise ValueError("one ratio per pilot bin")
    out = np.zeros(b.size, np.complex64)
    _arg_check(_L.orion_ofdm_interpolate_host(pb.ctypes.data, r.ctypes.data, pb.size, b.ctypes.data, b.size,
                                              out.ctypes.data))
    return out


class OfdmConfig:
    """OfdmConfig (src/python/ofdm.rs:50-130 over modulate/ofdm.rs:57-365): the carrier plan,
    sample rate, carrier, gain and constellation. With edge_guard the data carriers are the
    contiguous span of with_contiguous_data(edge_guard, False) and data_carriers must be empty.
    Raises ValueError as the reference does (validate), and for what this library does not
    take: an n_fft that is not a power of two from 8 to 4096, or cp_len > n_fft."""

    def __init__(self, n_fft, cp_len, data_carriers, pilot_carrier_indices, pilot_carrier_values, fs, rf_hz, gain,
                 constellation, edge_guard=None):
        data = _ofdm_arr(np.asarray(data_carriers), np.int32, "data_carriers") if not isinstance(data_carriers, np.ndarray) \
            else _ofdm_arr(data_carriers, np.int32, "data_carriers")
        pidx = _ofdm_arr(pilot_carrier_indices, np.int32, "pilot_carrier_indices")
        pval = _ofdm_arr(pilot_carrier_values, np.complex64, "pilot_carrier_values")
        if pidx.size != pval.size:
            raise ValueError(f"OfdmConfig: pilot_carrier_indices ({pidx.size}) and pilot_carrier_values ({pval.size}) "
                             "must have the same length")
        order = _ofdm_order(constellation)
        n_fft, cp_len = int(n_fft), int(cp_len)
        if n_fft < 8 or n_fft > 4096 or n_fft & (n_fft - 1):
            raise ValueError(f"OfdmConfig: n_fft {n_fft} is not a power of two from 8 to 4096")
        if cp_len < 0 or cp_len > n_fft:
            raise ValueError(f"OfdmConfig: cp_len {cp_len} outside 0..n_fft")
        if edge_guard is not None and data.size:
            raise ValueError("OfdmConfig: pass an empty data_carriers array when edge_guard is set "
                             "(the contiguous span is generated automatically)")
        self._h = _L.orion_ofdm_config_new(n_fft, cp_len, data.ctypes.data, data.size, pidx.ctypes.data,
                                           pval.ctypes.data, pidx.size, float(fs), float(rf_hz), float(gain), order)
        if not self._h:
            raise OrionError(f"orion_sdr: construction failed: {_err()}")
        if edge_guard is not None:
            _arg_check(_L.orion_ofdm_config_contiguous_data(self._h, int(edge_guard), 0))
        bad = C.c_int32(0)
        rc = _L.orion_ofdm_config_validate(self._h, -1, C.byref(bad))
        if rc > 0:
            raise ValueError(f"OfdmConfig: carrier plan error {OFDM_PLAN_ERRORS[rc]} (carrier index {bad.value})")
        _check(rc)
        self._args = (n_fft, cp_len, pidx.copy(), pval.copy(), float(fs), float(rf_hz), float(gain), constellation)
        self.constellation = constellation
        self.fs, self.rf_hz, self.gain = float(fs), float(rf_hz), float(gain)
        self.rx_window_backoff = 0
        self._frame = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _L is not None:
            _L.orion_ofdm_config_free(h)
            self._h = None

    def _info(self):
        a = (C.c_size_t * 8)()
        _check(_L.orion_ofdm_config_info(self._h, a))
        return [int(v) for v in a]

    n_fft = property(lambda self: self._info()[0])
    cp_len = property(lambda self: self._info()[1])
    num_data_carriers = property(lambda self: self._info()[2])
    bits_per_ofdm_symbol = property(lambda self: self._info()[4])
    samples_per_ofdm_symbol = property(lambda self: self._info()[5])
    occupied_half_carriers = property(lambda self: self._info()[6])
    window_roll_off = property(lambda self: self._info()[7])

    @property
    def data_carriers(self) -> np.ndarray:
        out = np.zeros(self._info()[2], np.int32)
        _check(_L.orion_ofdm_config_data_carriers(self._h, out.ctypes.data, out.size))
        return out

    def occupied_bins(self) -> np.ndarray:
        """occupied_bins (config.rs:188-203)."""
        out = np.zeros(self._info()[0], np.uint32)
        n = C.c_size_t(0)
        _check(_L.orion_ofdm_config_occupied_bins(self._h, out.ctypes.data, out.size, C.byref(n)))
        return out[: n.value].copy()

    def grid(self):
        """CarrierGrid::from_plan (grid.rs:40-66): (data_bins, pilot_bins) uint32."""
        i = self._info()
        d, p = np.zeros(i[2], np.uint32), np.zeros(i[3], np.uint32)
        _arg_check(_L.orion_ofdm_config_grid(self._h, d.ctypes.data, p.ctypes.data))
        return d, p

    def validate_edge_guard(self, edge_guard: int):
        """validate_edge_guard (config.rs:262-278): raises ValueError where it fails."""
        bad = C.c_int32(0)
        rc = _L.orion_ofdm_config_validate(self._h, int(edge_guard), C.byref(bad))
        if rc > 0:
            raise ValueError(f"OfdmConfig: carrier plan error {OFDM_PLAN_ERRORS[rc]} (carrier index {bad.value})")
        _check(rc)

    def _clone(self):
        n_fft, cp_len, pidx, pval, fs, rf, g, con = self._args
        c = OfdmConfig(n_fft, cp_len, self.data_carriers, pidx, pval, fs, rf, g, con)
        _check(_L.orion_ofdm_config_set_rx_window_backoff(c._h, self.rx_window_backoff))
        c.rx_window_backoff = self.rx_window_backoff
        _check(_L.orion_ofdm_config_set_symbol_window(c._h, self.window_roll_off))
        c._frame = dict(self.frame_fields)
        return c

    # ---- the frame-level fields (src/python/ofdm.rs:139-400 over modulate/ofdm.rs:100-340) ----
    _FRAME_DEFAULTS = {"payload_crc": "crc32", "header_crc": "crc16", "outer_interleaver": None,
                       "inner_interleaver": None, "scrambler": None, "scrambler_pos": "before_outer",
                       "header_format": "orion_sdr", "ldpc_decode_rule": "sum_product", "tx_lowpass": None}

    @property
    def frame_fields(self) -> dict:
        """The frame layer's settings with the reference's defaults: CRC-32 payload, CRC-16
        header, the OrionSdr header, no interleavers, no scrambler, sum-product, no TX low-pass."""
        return {**self._FRAME_DEFAULTS, **getattr(self, "_frame", {})}

    def _with_frame(self, **kw) -> "OfdmConfig":
        c = self._clone()
        c._frame.update(kw)
        c.validate_frame()
        return c

    def with_interleaver(self, stage, kind, a, b) -> "OfdmConfig":
        """with_block_interleaver / with_conv_interleaver: stage "inner" or "outer", kind "block"
        (rows, cols) or "forney" (branches, depth)."""
        if stage not in ("inner", "outer") or kind not in ("block", "forney"):
            raise ValueError('interleaver: stage "inner" / "outer", kind "block" / "forney"')
        return self._with_frame(**{stage + "_interleaver": (kind, int(a), int(b))})

    def with_payload_crc(self, crc) -> "OfdmConfig":
        return self._with_frame(payload_crc=crc)

    def with_header_crc(self, crc) -> "OfdmConfig":
        return self._with_frame(header_crc=crc)

    def with_scrambler(self, poly, width, seed=1, per_frame_random=False, position="before_outer") -> "OfdmConfig":
        return self._with_frame(scrambler=("additive", int(poly), int(width), "per_frame" if per_frame_random else int(seed)),
                                scrambler_pos=position)

    def with_dvbt_energy_dispersal(self) -> "OfdmConfig":
        return self._with_frame(scrambler="dvbt", scrambler_pos="before_outer")

    def with_header_format(self, fmt) -> "OfdmConfig":
        return self._with_frame(header_format=fmt)

    def with_ldpc_decode_rule(self, kind, scale=0.75) -> "OfdmConfig":
        return self._with_frame(ldpc_decode_rule=("scaled_min_sum", float(scale)) if kind == "scaled_min_sum" else kind)

    def with_tx_lowpass(self, lowpass) -> "OfdmConfig":
        """A TxLowpass, or None; applied last over the whole frame (host path only)."""
        if lowpass is not None and not isinstance(lowpass, TxLowpass):
            raise ValueError("tx_lowpass: a TxLowpass or None")
        return self._with_frame(tx_lowpass=lowpass)

    def validate_frame(self):
        """The frame checks of validate (modulate/ofdm.rs:320-340): nonzero interleaver
        dimensions, known kinds, and a per-frame seed needs a header to travel in. The header
        formats NoHeader and DvbTps are not built: they raise."""
        f = self.frame_fields
        for k in ("payload_crc", "header_crc"):
            if f[k] not in CRC_KINDS:
                raise ValueError(f"{k}: one of {sorted(CRC_KINDS)}")
        for k in ("outer_interleaver", "inner_interleaver"):
            if f[k] is not None and (f[k][1] <= 0 or f[k][2] <= 0):
                raise ValueError(f"{k}: dimensions must be nonzero")
        if f["header_format"] in ("none", "no_header", "dvb_tps", "dvbtps"):
            raise ValueError("header_format: only 'orion_sdr' is built (NoHeader and DvbTps are not)")
        if f["header_format"] not in ("orion_sdr", "orionsdr"):
            raise ValueError("header_format: 'orion_sdr'")
        if f["scrambler_pos"] not in ("before_outer", "after_inner"):
            raise ValueError('scrambler position: "before_outer" or "after_inner"')
        _ldpcf_rule(f["ldpc_decode_rule"])
        FrameScheme(crc=f["payload_crc"], outer_interleaver=f["outer_interleaver"],
                    inner_interleaver=f["inner_interleaver"], scrambler=f["scrambler"], scrambler_pos=f["scrambler_pos"])

    def symbol_config(self, constellation) -> "OfdmConfig":
        """symbol_config (modulate/ofdm_frame.rs:766-779): the bare per-symbol configuration of a
        constellation over this plan, the RX window back-off kept, no symbol window (the frame
        modulator tapers in its own post-pass, once)."""
        n_fft, cp_len, pidx, pval, fs, rf, g, _ = self._args
        c = OfdmConfig(n_fft, cp_len, self.data_carriers, pidx, pval, fs, rf, g, constellation)
        _check(_L.orion_ofdm_config_set_rx_window_backoff(c._h, self.rx_window_backoff))
        c.rx_window_backoff = self.rx_window_backoff
        return c

    def with_rx_window_backoff(self, backoff: int) -> "OfdmConfig":
        """with_rx_window_backoff (modulate/ofdm.rs:240-243): a new configuration."""
        if backoff < 0:
            raise ValueError("backoff must be >= 0")
        c = self._clone()
        _check(_L.orion_ofdm_config_set_rx_window_backoff(c._h, int(backoff)))
        c.rx_window_backoff = int(backoff)
        return c

    def with_symbol_window(self, roll_off: int) -> "OfdmConfig":
        """with_symbol_window (modulate/ofdm.rs:256-259): a new configuration."""
        if roll_off < 0:
            raise ValueError("roll_off must be >= 0")
        c = self._clone()
        _check(_L.orion_ofdm_config_set_symbol_window(c._h, int(roll_off)))
        return c


def _torch_1d(x, dtype_name, name):
    import torch

    if not x.is_cuda or not x.is_contiguous() or x.dim() != 1 or x.dtype != getattr(torch, dtype_name):
        raise ValueError(f"{name}: expected a 1-D contiguous {dtype_name} CUDA tensor")
    return x


class _FftBase:
    _inverse = False

    def __init__(self, n_fft: int):
        n_fft = int(n_fft)
        if n_fft < 8 or n_fft > 4096 or n_fft & (n_fft - 1):
            raise ValueError(f"{type(self).__name__}: n_fft {n_fft} is not a power of two from 8 to 4096")
        self._h = (_L.orion_ifft_new if self._inverse else _L.orion_fft_new)(n_fft)
        if not self._h:
            raise OrionError(f"orion_sdr: construction failed: {_err()}")
        self.n_fft = n_fft

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _L is not None:
            _L.orion_fft_free(h)
            self._h = None

    def process(self, x):
        """One n_fft-point symbol per call, as the reference block (fft.rs:42-54): the first
        n_fft values are transformed; a shorter input gives an empty array. numpy complex64
        in and out; a torch CUDA tensor stays resident."""
        if _is_torch(x):
            import torch

            x = _torch_1d(x, "complex64", "x")
            if x.numel() < self.n_fft:
                return torch.empty(0, dtype=torch.complex64, device=x.device)
            return self.process_batch(x[: self.n_fft].reshape(1, self.n_fft)).reshape(self.n_fft)
        x = _ofdm_arr(x, np.complex64, "x")
        out = np.zeros(self.n_fft, np.complex64)
        wr = WorkReport()
        _arg_check(_L.orion_fft_process(self._h, x.ctypes.data, x.size, out.ctypes.data, out.size, C.byref(wr)))
        return out[: wr.out_written]

    def process_batch(self, x, stream=None):
        """(batch, n_fft) symbols in one launch. A torch CUDA complex64 tensor whose rows are
        contiguous (any row stride >= n_fft, so a window of longer symbols may be passed as a
        view) stays resident; a numpy array costs one upload and one download."""
        import torch

        if not _is_torch(x):
            if not isinstance(x, np.ndarray) or x.dtype != np.complex64 or x.ndim != 2 or x.shape[1] != self.n_fft:
                raise ValueError(f"x: expected a (batch, {self.n_fft}) complex64 array")
            return self.process_batch(torch.from_numpy(np.ascontiguousarray(x)).cuda(), stream).cpu().numpy()
        if not x.is_cuda or x.dtype != torch.complex64 or x.dim() != 2 or x.shape[1] != self.n_fft or \
                (x.shape[0] > 0 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < self.n_fft):
            raise ValueError(f"x: expected a (batch, {self.n_fft}) complex64 CUDA tensor with contiguous rows")
        out = torch.empty((x.shape[0], self.n_fft), dtype=torch.complex64, device=x.device)
        stride = int(x.stride(0)) if x.shape[0] > 1 else self.n_fft
        _arg_check(_L.orion_fft_batch(self._h, x.data_ptr(), stride, out.data_ptr(), self.n_fft, int(x.shape[0]),
                                      SyncEngine._stream(x, stream)))
        return out


class FftBlock(_FftBase):
    """FftBlock (multicarrier/fft.rs:16-55) on the GPU: forward, unity gain."""


class IfftBlock(_FftBase):
    """IfftBlock (multicarrier/fft.rs:63-120) on the GPU: inverse, times 1 / n_fft."""
    _inverse = True


class _OfdmHandle:
    def __init__(self, h, cfg: OfdmConfig):
        if not h:
            msg = _err()
            raise ValueError(msg) if "ofdm" in msg else OrionError(f"orion_sdr: construction failed: {msg}")
        self._h = h
        self.bits_per_ofdm_symbol = cfg.bits_per_ofdm_symbol
        self.samples_per_ofdm_symbol = cfg.samples_per_ofdm_symbol
        self.num_data_carriers = cfg.num_data_carriers
        self.n_fft, self.cp_len = cfg.n_fft, cfg.cp_len

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _L is not None:
            _L.orion_ofdm_free(h)
            self._h = None

    def _process(self, x, out):
        wr = WorkReport()
        _arg_check(_L.orion_ofdm_process(self._h, x.ctypes.data, x.size, out.ctypes.data, out.size, C.byref(wr)))
        return wr

    def process_into(self, x, out) -> WorkReport:
        """The Block contract (core.rs:12-22) on the GPU: as many whole symbols as fit in both."""
        return self._process(_ofdm_arr(x, self._in, "input"), _ofdm_arr(out, self._out, "output"))

    def process_host_into(self, x, out) -> WorkReport:
        """The same call through the library's scalar host code (no device)."""
        x, out = _ofdm_arr(x, self._in, "input"), _ofdm_arr(out, self._out, "output")
        wr = WorkReport()
        _arg_check(self._host_fn(self._h, x.ctypes.data, x.size, out.ctypes.data, out.size, C.byref(wr)))
        return wr


class OfdmMod(_OfdmHandle):
    """OfdmMod (modulate/ofdm.rs:422-544; src/python/ofdm.rs) on the GPU: bits -> mapper -> grid
    -> inverse transform -> cyclic prefix -> optional symbol window -> gain (and the rotator
    when rf_hz != 0, whose phase carries across calls), one launch for every symbol."""
    _in, _out = np.uint8, np.complex64
    _host_fn = staticmethod(lambda *a: _L.orion_ofdm_mod_host(*a))

    def __init__(self, cfg: OfdmConfig):
        super().__init__(_L.orion_ofdm_mod_new(cfg._h), cfg)

    def set_gain(self, g: float):
        _check(_L.orion_ofdm_set_gain(self._h, float(g)))

    def reset(self):
        _check(_L.orion_ofdm_reset(self._h))

    def modulate(self, bits):
        """modulate (modulate/ofdm.rs:469-493): every bit, the last symbol zero-padded. uint8
        numpy bits -> numpy complex64; a torch CUDA uint8 tensor stays resident."""
        bps = self.bits_per_ofdm_symbol
        if _is_torch(bits):
            import torch

            bits = _torch_1d(bits, "uint8", "bits")
            nsym = -(-bits.numel() // bps)
            if nsym * bps != bits.numel():
                bits = torch.cat([bits, torch.zeros(nsym * bps - bits.numel(), dtype=torch.uint8, device=bits.device)])
            return ofdm_modulate_batch(self, bits.reshape(1, -1)).reshape(-1)
        bits = _ofdm_arr(bits, np.uint8, "bits")
        nsym = -(-bits.size // bps)
        padded = np.zeros(nsym * bps, np.uint8)
        padded[: bits.size] = bits
        out = np.zeros(nsym * self.samples_per_ofdm_symbol, np.complex64)
        self._process(padded, out)
        return out

    def modulate_host(self, bits) -> np.ndarray:
        """modulate by the library's scalar host code (what the kernels are held to)."""
        bits = _ofdm_arr(bits, np.uint8, "bits")
        nsym = -(-bits.size // self.bits_per_ofdm_symbol)
        padded = np.zeros(nsym * self.bits_per_ofdm_symbol, np.uint8)
        padded[: bits.size] = bits
        out = np.zeros(nsym * self.samples_per_ofdm_symbol, np.complex64)
        self.process_host_into(padded, out)
        return out


class OfdmDecider(_OfdmHandle):
    """OfdmDecider (demodulate/ofdm.rs:137-166) on the GPU: soft symbols -> hard bits."""
    _in, _out = np.complex64, np.uint8

    def __init__(self, cfg: OfdmConfig):
        super().__init__(_L.orion_ofdm_decider_new(cfg._h), cfg)
        self._order = _ofdm_order(cfg.constellation)

    def process(self, soft):
        if _is_torch(soft):
            import torch

            soft = _torch_1d(soft, "complex64", "soft")
            k = soft.numel() // self.num_data_carriers
            out = torch.empty(k * self.bits_per_ofdm_symbol, dtype=torch.uint8, device=soft.device)
            _arg_check(_L.orion_ofdm_decider_device(self._h, soft.data_ptr(), 1, k, out.data_ptr(),
                                                    SyncEngine._stream(soft, None)))
            return out
        soft = _ofdm_arr(soft, np.complex64, "soft")
        out = np.zeros(soft.size // self.num_data_carriers * self.bits_per_ofdm_symbol, np.uint8)
        self._process(soft, out)
        return out

    def process_host(self, soft) -> np.ndarray:
        soft = _ofdm_arr(soft, np.complex64, "soft")
        k = soft.size // self.num_data_carriers
        return ofdm_decide(self._constellation_name(), soft[: k * self.num_data_carriers])

    def _constellation_name(self):
        return [k for k, v in OFDM_CONSTELLATIONS.items() if v == self._order][0]


class OfdmSoftDemod(_OfdmHandle):
    """OfdmSoftDemod (demodulate/ofdm.rs:693-731) on the GPU: soft symbols -> max-log LLRs."""
    _in, _out = np.complex64, np.float32

    def __init__(self, cfg: OfdmConfig):
        super().__init__(_L.orion_ofdm_soft_demod_new(cfg._h), cfg)
        self._constellation = cfg.constellation

    def process(self, soft):
        if _is_torch(soft):
            import torch

            soft = _torch_1d(soft, "complex64", "soft")
            k = soft.numel() // self.num_data_carriers
            out = torch.empty(k * self.bits_per_ofdm_symbol, dtype=torch.float32, device=soft.device)
            _arg_check(_L.orion_ofdm_soft_demod_device(self._h, soft.data_ptr(), 1, k, out.data_ptr(),
                                                       SyncEngine._stream(soft, None)))
            return out
        soft = _ofdm_arr(soft, np.complex64, "soft")
        out = np.zeros(soft.size // self.num_data_carriers * self.bits_per_ofdm_symbol, np.float32)
        self._process(soft, out)
        return out

    def process_host(self, soft) -> np.ndarray:
        soft = _ofdm_arr(soft, np.complex64, "soft")
        k = soft.size // self.num_data_carriers
        return ofdm_llr(self._constellation, soft[: k * self.num_data_carriers])


class OfdmEqualizer(_OfdmHandle):
    """OfdmEqualizer (demodulate/ofdm.rs:333-569) on the GPU over whole n_fft-bin vectors:
    method "training_symbol" (estimate once, hold) or "pilot_interp" (per symbol, linear
    between the pilots, by binary search per bin)."""
    _in, _out = np.complex64, np.complex64
    _host_fn = staticmethod(lambda *a: _L.orion_ofdm_equalize_host(*a))

    def __init__(self, cfg: OfdmConfig, method: str = "training_symbol"):
        if method not in ("training_symbol", "pilot_interp"):
            raise ValueError(f"OfdmEqualizer: unknown method {method!r} (expected 'training_symbol' or 'pilot_interp')")
        super().__init__(_L.orion_ofdm_equalizer_new(cfg._h, _OFDM_EQ[method]), cfg)
        self.method = method

    def estimate_from_training_symbol(self, received_freq):
        """estimate_from_training_symbol (demodulate/ofdm.rs:440-448): n_fft received bins."""
        r = _ofdm_arr(received_freq, np.complex64, "received_freq")
        _arg_check(_L.orion_ofdm_estimate_channel(self._h, r.ctypes.data, r.size))

    def set_pilot_bins(self, pilot_bins, pilot_values, data_bins):
        """set_pilot_bins (demodulate/ofdm.rs:426-432)."""
        pb, db = np.ascontiguousarray(pilot_bins, np.uint32), np.ascontiguousarray(data_bins, np.uint32)
        pv = _ofdm_arr(pilot_values, np.complex64, "pilot_values")
        if pb.size != pv.size:
            raise ValueError("one value per pilot bin")
        _arg_check(_L.orion_ofdm_set_pilot_bins_host(self._h, pb.ctypes.data, pv.ctypes.data, pb.size, db.ctypes.data,
                                                     db.size))

    def process(self, freq):
        if _is_torch(freq):
            import torch

            freq = _torch_1d(freq, "complex64", "freq")
            k = freq.numel() // self.n_fft
            out = torch.empty(k * self.n_fft, dtype=torch.complex64, device=freq.device)
            _arg_check(_L.orion_ofdm_equalizer_device(self._h, freq.data_ptr(), 1, k, out.data_ptr(),
                                                      SyncEngine._stream(freq, None)))
            return out
        freq = _ofdm_arr(freq, np.complex64, "freq")
        out = np.zeros(freq.size // self.n_fft * self.n_fft, np.complex64)
        self._process(freq, out)
        return out

    def process_host(self, freq) -> np.ndarray:
        freq = _ofdm_arr(freq, np.complex64, "freq")
        out = np.zeros(freq.size // self.n_fft * self.n_fft, np.complex64)
        self.process_host_into(freq, out)
        return out


class OfdmDemod(_OfdmHandle):
    """OfdmDemod (demodulate/ofdm.rs:26-95 with SymbolFft's window back-off; src/python/ofdm.rs:
    506-631) on the GPU: window select -> forward transform -> equalizer -> grid gather ->
    gain, hard bits from the same launch. equalizer "training_symbol" (identity until
    estimate_channel), "pilot_interp", or None for the bare Rust block.

    One stated divergence: the reference's Python demodulate reads only the first symbol of
    its input (src/python/ofdm.rs:607-630); this one reads every whole symbol. For a
    one-symbol input the two agree."""
    _in, _out = np.complex64, np.complex64
    _host_fn = staticmethod(lambda *a: _L.orion_ofdm_demod_host(*a))

    def __init__(self, cfg: OfdmConfig, equalizer="training_symbol"):
        if equalizer not in _OFDM_EQ:
            raise ValueError(f"OfdmDemod: unknown equalizer {equalizer!r} (expected 'training_symbol' or 'pilot_interp')")
        super().__init__(_L.orion_ofdm_demod_new(cfg._h, _OFDM_EQ[equalizer]), cfg)
        self.equalizer = equalizer
        self._start = cfg.cp_len - min(cfg.rx_window_backoff, cfg.cp_len)
        self._fft = None

    def set_gain(self, g: float):
        _check(_L.orion_ofdm_set_gain(self._h, float(g)))

    def estimate_channel(self, training_iq):
        """estimate_channel (src/python/ofdm.rs:563-582): one received training symbol's IQ
        (cyclic prefix included) -> the held channel estimate; the window is the demodulator's
        own (the configuration's back-off). A no-op under "pilot_interp"."""
        if self.equalizer is None:
            raise ValueError("OfdmDemod.estimate_channel: this demodulator has no equalizer")
        iq = _ofdm_arr(training_iq, np.complex64, "training_iq")
        if iq.size < self.samples_per_ofdm_symbol:
            raise ValueError(f"OfdmDemod.estimate_channel: input too short ({iq.size} < {self.samples_per_ofdm_symbol})")
        if self._fft is None:
            self._fft = FftBlock(self.n_fft)
        freq = self._fft.process(np.ascontiguousarray(iq[self._start: self._start + self.n_fft]))
        _arg_check(_L.orion_ofdm_estimate_channel(self._h, freq.ctypes.data, freq.size))

    def estimate_channel_freq(self, received_freq):
        """The same from the training symbol's n_fft received bins."""
        r = _ofdm_arr(received_freq, np.complex64, "received_freq")
        if self.equalizer is None:
            raise ValueError("OfdmDemod.estimate_channel: this demodulator has no equalizer")
        _arg_check(_L.orion_ofdm_estimate_channel(self._h, r.ctypes.data, r.size))

    def demodulate_soft(self, iq):
        """(soft symbols, hard bits) of every whole symbol of iq."""
        if _is_torch(iq):
            iq = _torch_1d(iq, "complex64", "iq")
            if iq.numel() < self.samples_per_ofdm_symbol:
                raise ValueError(f"OfdmDemod.demodulate: input too short ({iq.numel()} < {self.samples_per_ofdm_symbol})")
            k = iq.numel() // self.samples_per_ofdm_symbol
            soft, bits, _ = ofdm_demodulate_batch(self, iq[: k * self.samples_per_ofdm_symbol].reshape(1, -1))
            return soft.reshape(-1), bits.reshape(-1)
        iq = _ofdm_arr(iq, np.complex64, "iq")
        if iq.size < self.samples_per_ofdm_symbol:
            raise ValueError(f"OfdmDemod.demodulate: input too short ({iq.size} < {self.samples_per_ofdm_symbol})")
        k = iq.size // self.samples_per_ofdm_symbol
        soft, bits, _ = ofdm_demodulate_batch(self, iq[: k * self.samples_per_ofdm_symbol].reshape(1, -1))
        return soft.reshape(-1), bits.reshape(-1)

    def demodulate(self, iq):
        return self.demodulate_soft(iq)[1]

    def process(self, iq) -> np.ndarray:
        """The Block contract: numpy IQ -> the soft symbols of every whole symbol."""
        iq = _ofdm_arr(iq, np.complex64, "iq")
        out = np.zeros(iq.size // self.samples_per_ofdm_symbol * self.num_data_carriers, np.complex64)
        self._process(iq, out)
        return out

    def process_host(self, iq) -> np.ndarray:
        iq = _ofdm_arr(iq, np.complex64, "iq")
        out = np.zeros(iq.size // self.samples_per_ofdm_symbol * self.num_data_carriers, np.complex64)
        self.process_host_into(iq, out)
        return out

    def equalize_track(self, raw, weights, n_symbols, llr=True, stream=None):
        """The equalizer branch of the frame demodulator's soft_demap on the GPU, for frames of
        n_symbols symbols: raw (frames, n_symbols * data carriers) soft symbols of a
        demodulator with no equalizer and gain 1, weights (frames, n_fft) per-frame equalizer
        coefficients -> (symbols after the common-phase-error tracker, their LLRs or None).
        Contiguous complex64 CUDA tensors, queued on torch's current stream or on stream."""
        import torch

        for t, w in ((raw, n_symbols * self.num_data_carriers), (weights, self.n_fft)):
            if not _is_torch(t) or not t.is_cuda or not t.is_contiguous() or t.dtype != torch.complex64 or t.dim() != 2 \
                    or int(t.shape[1]) != w or int(t.shape[0]) != int(raw.shape[0]):
                raise ValueError("equalize_track: contiguous complex64 CUDA tensors (frames, n_symbols * data carriers) "
                                 "and (frames, n_fft)")
        syms = torch.empty_like(raw)
        out = torch.empty((raw.shape[0], n_symbols * self.bits_per_ofdm_symbol), dtype=torch.float32, device=raw.device) \
            if llr else None
        _arg_check(_L.orion_ofdm_equalize_track_device(self._h, raw.data_ptr(), weights.data_ptr(), int(raw.shape[0]),
                                                       int(n_symbols), syms.data_ptr(), out.data_ptr() if llr else None,
                                                       SyncEngine._stream(raw, stream)))
        return syms, out


def ofdm_modulate_batch(mod: OfdmMod, bits, stream=None):
    """n_channels x n_symbols symbols in one launch: uint8 (n_channels, n_symbols *
    bits_per_ofdm_symbol) -> complex64 (n_channels, n_symbols * samples_per_ofdm_symbol). A
    numpy array costs one upload and one download; a torch CUDA tensor stays resident (queued
    on torch's current stream or on stream). With rf_hz != 0 every channel continues the
    modulator's rotator from the same phase."""
    import torch

    if not _is_torch(bits):
        if not isinstance(bits, np.ndarray) or bits.dtype != np.uint8 or bits.ndim != 2:
            raise ValueError("bits: expected a 2-D uint8 array")
        return ofdm_modulate_batch(mod, torch.from_numpy(np.ascontiguousarray(bits)).cuda(), stream).cpu().numpy()
    if not bits.is_cuda or not bits.is_contiguous() or bits.dtype != torch.uint8 or bits.dim() != 2:
        raise ValueError("bits: expected a contiguous 2-D uint8 CUDA tensor")
    nch, nb = int(bits.shape[0]), int(bits.shape[1])
    if nb % mod.bits_per_ofdm_symbol:
        raise ValueError(f"bits: {nb} per channel is not a whole number of symbols ({mod.bits_per_ofdm_symbol} bits each)")
    nsym = nb // mod.bits_per_ofdm_symbol
    out = torch.empty((nch, nsym * mod.samples_per_ofdm_symbol), dtype=torch.complex64, device=bits.device)
    _arg_check(_L.orion_ofdm_mod_device(mod._h, bits.data_ptr(), nch, nsym, out.data_ptr(),
                                        SyncEngine._stream(bits, stream)))
    return out


def ofdm_demodulate_batch(demod: OfdmDemod, iq, bits=True, llr=False, stream=None):
    """n_channels x n_symbols symbols in one launch: complex64 (n_channels, n_symbols *
    samples_per_ofdm_symbol) -> (soft complex64 (n_channels, n_symbols * data carriers), bits
    uint8 or None, llr float32 or None), the last two (n_channels, n_symbols *
    bits_per_ofdm_symbol). numpy in, numpy out (one upload); torch CUDA tensors stay resident."""
    import torch

    if not _is_torch(iq):
        if not isinstance(iq, np.ndarray) or iq.dtype != np.complex64 or iq.ndim != 2:
            raise ValueError("iq: expected a 2-D complex64 array")
        r = ofdm_demodulate_batch(demod, torch.from_numpy(np.ascontiguousarray(iq)).cuda(), bits, llr, stream)
        return tuple(None if t is None else t.cpu().numpy() for t in r)
    if not iq.is_cuda or not iq.is_contiguous() or iq.dtype != torch.complex64 or iq.dim() != 2:
        raise ValueError("iq: expected a contiguous 2-D complex64 CUDA tensor")
    nch, n = int(iq.shape[0]), int(iq.shape[1])
    if n % demod.samples_per_ofdm_symbol:
        raise ValueError(f"iq: {n} per channel is not a whole number of symbols ({demod.samples_per_ofdm_symbol} samples each)")
    nsym = n // demod.samples_per_ofdm_symbol
    soft = torch.empty((nch, nsym * demod.num_data_carriers), dtype=torch.complex64, device=iq.device)
    b = torch.empty((nch, nsym * demod.bits_per_ofdm_symbol), dtype=torch.uint8, device=iq.device) if bits else None
    l = torch.empty((nch, nsym * demod.bits_per_ofdm_symbol), dtype=torch.float32, device=iq.device) if llr else None
    _arg_check(_L.orion_ofdm_demod_device(demod._h, iq.data_ptr(), nch, nsym, soft.data_ptr(),
                                          b.data_ptr() if bits else None, l.data_ptr() if llr else None,
                                          SyncEngine._stream(iq, stream)))
    return soft, b, l


class OfdmRxFrame:
    """OfdmRxFrame (demodulate/ofdm.rs:173-226; src/python/ofdm.rs:637-673): the symbol layer
    fills bits, num_symbols and evm_db; every other field is None."""

    def __init__(self, bits, num_symbols, evm_db):
        self.bits, self.num_symbols, self.evm_db = bits, num_symbols, evm_db
        self.cfo_hz = self.timing_offset_samples = self.channel_mse = None
        self.sync_score = self.channel_estimate = self.inner_fec_ok = self.outer_fec_ok = None
        self.channel_ber = self.inner_ber = None


def build_ofdm_rx_frame(cfg: OfdmConfig, soft_symbols, bits) -> OfdmRxFrame:
    """build_ofdm_rx_frame (demodulate/ofdm.rs:238-293): EVM of the soft symbols against the
    ideal points of the hard bits, f64 sums (host only)."""
    soft = _ofdm_arr(soft_symbols, np.complex64, "soft_symbols")
    bits = _ofdm_arr(bits, np.uint8, "bits")
    nd = cfg.num_data_carriers
    nsym = soft.size // nd if nd else 0
    evm, valid = C.c_float(0.0), C.c_int(0)
    _check(_L.orion_ofdm_evm_db_host(_ofdm_order(cfg.constellation), soft.ctypes.data, soft.size, bits.ctypes.data,
                                     bits.size, nsym, C.byref(evm), C.byref(valid)))
    return OfdmRxFrame(bits.copy(), nsym, float(evm.value) if valid.value else None)


# ---- the inner code: punctured convolutional code, soft Viterbi, block interleaver (src/fec) ----
def _fec_sigs():
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    sig = {
        "orion_fec_punctured_coded_len": (sz, [i, sz, i]), "orion_fec_encoded_len": (sz, [i, sz, i, sz, sz]),
        "orion_fec_conv_encode": (i, [i, i, vp, sz, vp]),
        "orion_fec_viterbi_host": (i, [i, i, vp, sz, sz, sz, sz, vp]),
        "orion_fec_viterbi": (i, [i, i, vp, sz, sz, sz, sz, sz, vp]),
        "orion_fec_viterbi_device": (i, [i, i, vp, sz, sz, sz, sz, sz, vp, vp, sz, vp]),
        "orion_fec_viterbi_work_bytes": (sz, [i, sz, sz]),
        "orion_fec_conv_encode_batch": (i, [i, i, vp, sz, sz, sz, sz, vp]),
        "orion_fec_conv_encode_batch_device": (i, [i, i, vp, sz, sz, sz, sz, vp, vp]),
        "orion_fec_interleave_u8": (i, [sz, sz, vp, vp]), "orion_fec_interleave_f32": (i, [sz, sz, vp, vp]),
        "orion_fec_deinterleave_u8": (i, [sz, sz, vp, vp]), "orion_fec_deinterleave_f32": (i, [sz, sz, vp, vp]),
        "orion_fec_interleaved_len": (sz, [sz, sz, sz]),
        "orion_fec_interleave_bits": (i, [sz, sz, vp, sz, vp]),
        "orion_fec_deinterleave_llrs": (i, [sz, sz, vp, sz, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(_L, name)
        fn.restype = res
        fn.argtypes = args


_fec_sigs()

FEC_CODES = {"k5": 0, "dvb_k7": 1}  # conv.rs:41-50
FEC_RATES = {"1/2": 0, "2/3": 1, "3/4": 2, "5/6": 3, "7/8": 4}  # conv.rs:99-106
__all__ += ["FEC_CODES", "FEC_RATES", "punctured_coded_len", "conv_encode_punctured", "viterbi_decode_soft",
            "BlockInterleaver", "conv_encode_batch", "conv_viterbi_batch"]


def _fec_code(code) -> int:
    if code not in FEC_CODES:
        raise ValueError(f"code: one of {sorted(FEC_CODES)}")
    return FEC_CODES[code]


def _fec_rate(rate) -> int:
    if rate not in FEC_RATES:
        raise ValueError(f"rate: one of {list(FEC_RATES)}")
    return FEC_RATES[rate]


def _fec_il(interleaver):
    if interleaver is None:
        return 0, 0
    if isinstance(interleaver, BlockInterleaver):
        return interleaver.rows, interleaver.cols
    rows, cols = interleaver
    return BlockInterleaver(rows, cols).rows, int(cols)


def _fec_info_bits(info_bits) -> int:
    info_bits = int(info_bits)
    if info_bits < 1:
        raise ValueError("info_bits: at least 1")
    return info_bits


def punctured_coded_len(info_bits, rate, code="k5") -> int:
    """punctured_coded_len_with (conv.rs:274-288): the coded bits of info_bits information
    bits and the K - 1 tail bits at rate "1/2" .. "7/8" under code "k5" / "dvb_k7"."""
    c, r, n = _fec_code(code), _fec_rate(rate), _fec_info_bits(info_bits)
    out = int(_L.orion_fec_punctured_coded_len(c, n, r))
    if out == 0:
        raise ValueError(_err())
    return out


def conv_encode_punctured(bits, rate, code="k5") -> np.ndarray:
    """conv_encode_punctured_with (conv.rs:234-263), host only: uint8 information bits (n,) ->
    coded bits (punctured_coded_len(n, rate, code),): the zero tail, the mother code's (g0, g1)
    pairs, the rate's puncturing."""
    bits = _bits_arg(bits)
    out = np.zeros(punctured_coded_len(bits.size, rate, code), np.uint8)
    _arg_check(_L.orion_fec_conv_encode(_fec_code(code), _fec_rate(rate), bits.ctypes.data, bits.size, out.ctypes.data))
    return out


def viterbi_decode_soft(llr, info_bits, rate, code="k5") -> np.ndarray:
    """viterbi_decode_soft_with (conv.rs:304-398) by the library's scalar decoder (host only;
    what the kernel is held to): float32 LLRs (n_llr,) in punctured order, positive meaning
    bit 0 -> uint8 bits (info_bits,). LLRs past n_llr read as 0.0."""
    if not isinstance(llr, np.ndarray) or llr.dtype != np.float32 or llr.ndim != 1:
        raise ValueError("llr: expected a 1-D float32 array")
    llr = np.ascontiguousarray(llr)
    out = np.zeros(_fec_info_bits(info_bits), np.uint8)
    _arg_check(_L.orion_fec_viterbi_host(_fec_code(code), _fec_rate(rate), llr.ctypes.data, llr.size, out.size, 0, 0,
                                         out.ctypes.data))
    return out


class BlockInterleaver:
    """BlockInterleaver (fec/interleaver.rs:53-120), host only: interleave / deinterleave take
    one block of rows * cols uint8 or float32 elements (out[c rows + r] = in[r cols + c] and
    its inverse); interleave_bits and deinterleave_llrs are the frame chain's drivers
    (modulate/ofdm_frame.rs, demodulate/ofdm_frame.rs): the first zero-pads the last block,
    the second leaves a short last chunk as it is."""

    def __init__(self, rows, cols):
        rows, cols = int(rows), int(cols)
        if rows < 1 or cols < 1:
            raise ValueError("interleaver dimensions must be nonzero")
        if rows * cols > 1 << 24:
            raise ValueError("interleaver: rows * cols above 2^24")
        self.rows, self.cols = rows, cols

    @property
    def block_len(self) -> int:
        return self.rows * self.cols

    def _block(self, x, inverse):
        if not isinstance(x, np.ndarray) or x.dtype not in (np.uint8, np.float32) or x.ndim != 1:
            raise ValueError("expected a 1-D uint8 or float32 array")
        if x.size != self.block_len:
            raise ValueError(f"expected one full block of {self.block_len} elements")
        x = np.ascontiguousarray(x)
        out = np.empty_like(x)
        name = f"orion_fec_{'de' if inverse else ''}interleave_{'u8' if x.dtype == np.uint8 else 'f32'}"
        _arg_check(getattr(_L, name)(self.rows, self.cols, x.ctypes.data, out.ctypes.data))
        return out

    def interleave(self, x) -> np.ndarray:
        return self._block(x, False)

    def deinterleave(self, x) -> np.ndarray:
        return self._block(x, True)

    def interleave_bits(self, bits) -> np.ndarray:
        bits = _bits_arg(bits)
        out = np.zeros(int(_L.orion_fec_interleaved_len(self.rows, self.cols, bits.size)), np.uint8)
        _arg_check(_L.orion_fec_interleave_bits(self.rows, self.cols, bits.ctypes.data, bits.size, out.ctypes.data))
        return out

    def deinterleave_llrs(self, llr) -> np.ndarray:
        if not isinstance(llr, np.ndarray) or llr.dtype != np.float32 or llr.ndim != 1:
            raise ValueError("llr: expected a 1-D float32 array")
        llr = np.ascontiguousarray(llr)
        out = np.zeros(llr.size, np.float32)
        _arg_check(_L.orion_fec_deinterleave_llrs(self.rows, self.cols, llr.ctypes.data, llr.size, out.ctypes.data))
        return out


def conv_encode_batch(bits, rate, code="k5", interleaver=None, stream=None):
    """Encode, puncture and (with interleaver, a BlockInterleaver or (rows, cols)) block
    interleave a batch of frames on the GPU in one launch: uint8 (nstreams, info_bits) ->
    uint8 (nstreams, coded length), the coded length rounded up to whole interleaver blocks
    (zero padding). Row k is interleave_bits(conv_encode_punctured(bits[k])). A numpy array
    (-> numpy) or a contiguous torch CUDA tensor (-> a torch tensor on its device, queued on
    torch's current stream or on stream)."""
    c, r = _fec_code(code), _fec_rate(rate)
    rows, cols = _fec_il(interleaver)
    dev = _is_torch(bits)
    if dev:
        import torch

        if not bits.is_cuda or not bits.is_contiguous() or bits.dtype != torch.uint8 or bits.dim() != 2:
            raise ValueError("conv_encode_batch needs a contiguous 2-D uint8 CUDA tensor")
    elif not isinstance(bits, np.ndarray) or bits.dtype != np.uint8 or bits.ndim != 2:
        raise ValueError("bits: expected a 2-D uint8 array")
    ns, n = int(bits.shape[0]), _fec_info_bits(bits.shape[1])
    out_len = int(_L.orion_fec_encoded_len(c, n, r, rows, cols))
    if out_len == 0:
        raise ValueError(_err())
    if dev:
        out = torch.empty((ns, out_len), dtype=torch.uint8, device=bits.device)
        _arg_check(_L.orion_fec_conv_encode_batch_device(c, r, bits.data_ptr(), ns, n, rows, cols, out.data_ptr(),
                                                         SyncEngine._stream(bits, stream)))
        return out
    bits = np.ascontiguousarray(bits)
    out = np.zeros((ns, out_len), np.uint8)
    _arg_check(_L.orion_fec_conv_encode_batch(c, r, bits.ctypes.data, ns, n, rows, cols, out.ctypes.data))
    return out


def conv_viterbi_batch(llr, info_bits, rate, code="k5", interleaver=None, stream=None):
    """Soft Viterbi decode of a batch of frames on the GPU in one launch (one lane per trellis
    state: "dvb_k7" one frame per wave, "k5" four), the block deinterleaver and the
    depuncturing fused into the LLR fetch: float32 (nstreams, n_llr), positive meaning bit 0,
    -> uint8 (nstreams, info_bits). Row k is viterbi_decode_soft(deinterleave_llrs(llr[k]),
    info_bits, rate, code) bit for bit. A numpy array (-> numpy) or a contiguous torch CUDA
    tensor, such as the llr of ofdm_demodulate_batch(..., llr=True) (-> a torch tensor on its
    device, queued on torch's current stream or on stream)."""
    c, r, n = _fec_code(code), _fec_rate(rate), _fec_info_bits(info_bits)
    rows, cols = _fec_il(interleaver)
    if _is_torch(llr):
        import torch

        if not llr.is_cuda or not llr.is_contiguous() or llr.dtype != torch.float32 or llr.dim() != 2:
            raise ValueError("conv_viterbi_batch needs a contiguous 2-D float32 CUDA tensor")
        ns, nl = int(llr.shape[0]), int(llr.shape[1])
        bits = torch.empty((ns, n), dtype=torch.uint8, device=llr.device)
        wb = int(_L.orion_fec_viterbi_work_bytes(c, ns, n))
        work = torch.empty(max(wb // 8, 1), dtype=torch.int64, device=llr.device)
        _arg_check(_L.orion_fec_viterbi_device(c, r, llr.data_ptr(), ns, nl, n, rows, cols, bits.data_ptr(),
                                               work.data_ptr(), wb, SyncEngine._stream(llr, stream)))
        return bits
    if not isinstance(llr, np.ndarray) or llr.dtype != np.float32 or llr.ndim != 2:
        raise ValueError("llr: expected a 2-D float32 array")
    llr = np.ascontiguousarray(llr)
    ns, nl = llr.shape
    bits = np.zeros((ns, n), np.uint8)
    _arg_check(_L.orion_fec_viterbi(c, r, llr.ctypes.data, ns, nl, n, rows, cols, bits.ctypes.data))
    return bits


# ---- the outer code: Reed-Solomon, the Forney interleaver, scramblers, the TS layer (src/fec,
# src/waveform/dvb_t.rs, dvb_t_ts.rs) ----
def _rs_sigs():
    vp, sz, i, u, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_uint32
    sig = {
        "orion_rs_gf_tables": (i, [vp, vp]), "orion_rs_gf_mul": (i, [u, u]), "orion_rs_gf_div": (i, [u, u]),
        "orion_rs_gf_inv": (i, [u]), "orion_rs_gf_pow": (i, [u, sz]), "orion_rs_gf_exp_of": (i, [sz]),
        "orion_rs_generator": (i, [sz, sz, vp]), "orion_rs_encode": (i, [sz, sz, vp, sz, vp]),
        "orion_rs_decode_counted": (i, [sz, sz, vp, sz, vp, vp]),
        "orion_rs_forney_new": (vp, [sz, sz, i]), "orion_rs_forney_free": (None, [vp]),
        "orion_rs_forney_feed": (i, [vp, vp, sz, vp]), "orion_rs_forney_flush": (i, [vp, vp]),
        "orion_rs_forney_reset": (i, [vp]), "orion_rs_forney_delay": (sz, [sz, sz]),
        "orion_rs_forney_frame_len": (sz, [sz, sz, sz]),
        "orion_rs_forney_frame_interleave": (i, [sz, sz, vp, sz, vp]),
        "orion_rs_forney_frame_deinterleave": (i, [sz, sz, vp, sz, vp]),
        "orion_rs_pn_scramble": (i, [u32, u32, u32, vp, sz]),
        "orion_rs_pn_stream_new": (vp, [u32, u32, u32]), "orion_rs_pn_stream_free": (None, [vp]),
        "orion_rs_pn_stream_feed": (i, [vp, vp, sz]), "orion_rs_pn_stream_reset": (i, [vp]),
        "orion_rs_dispersal_new": (vp, []), "orion_rs_dispersal_free": (None, [vp]),
        "orion_rs_dispersal_feed": (i, [vp, vp, sz]), "orion_rs_dispersal_advance_byte": (i, [vp]),
        "orion_rs_dispersal_reset": (i, [vp]),
        "orion_rs_ts_energy_disperse": (i, [vp, sz]), "orion_rs_ts_dispersal_mask": (i, [vp]),
        "orion_rs_ts_packetized_len": (sz, [sz]), "orion_rs_ts_packetize": (i, [vp, sz, vp]),
        "orion_rs_ts_depacketize": (i, [vp, sz, vp]), "orion_rs_ts_null_packet": (i, [vp]),
        "orion_rs_ts_stuff_null_packets": (i, [vp, sz, sz, vp]),
        "orion_rs_decode_stream_len": (sz, [sz, sz, sz, i, sz, sz]),
        "orion_rs_decode_batch": (i, [sz, sz, vp, sz, sz, i, sz, sz, i, vp, vp]),
        "orion_rs_decode_batch_device": (i, [sz, sz, vp, sz, sz, i, sz, sz, i, vp, vp, vp]),
        "orion_rs_encode_batch": (i, [sz, sz, vp, sz, sz, i, vp]),
        "orion_rs_encode_batch_device": (i, [sz, sz, vp, sz, sz, i, vp, vp]),
        "orion_rs_forney_interleave_len": (sz, [sz, sz, sz, i]),
        "orion_rs_forney_interleave_batch": (i, [sz, sz, vp, sz, sz, i, vp]),
        "orion_rs_forney_interleave_batch_device": (i, [sz, sz, vp, sz, sz, i, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(_L, name)
        fn.restype = res
        fn.argtypes = args


_rs_sigs()

__all__ += ["Gf256", "ReedSolomon", "RsUncorrectable", "ConvInterleaver", "ConvDeinterleaver", "PnScrambler",
            "PnScramblerStream", "DvbTEnergyDispersal", "forney_frame_interleave", "forney_frame_deinterleave",
            "ts_energy_disperse", "ts_packetize", "ts_depacketize", "ts_null_packet", "ts_stuff_null_packets",
            "rs_encode_batch", "rs_decode_batch", "forney_interleave_batch", "TS_PACKET_LEN"]
TS_PACKET_LEN = 188


def _bytes_arg(x, what="data", ndim=1) -> np.ndarray:
    if isinstance(x, (bytes, bytearray)) and ndim == 1:
        x = np.frombuffer(bytes(x), np.uint8)
    if not isinstance(x, np.ndarray) or x.dtype != np.uint8 or x.ndim != ndim:
        raise ValueError(f"{what}: expected a {ndim}-D uint8 array")
    return np.ascontiguousarray(x)


def _gf_elem(rc: int) -> int:
    if rc < 0:
        raise ValueError(_err())
    return rc


class Gf256:
    """GF(2^8) under 0x11D with generator 2 (fec/gf.rs), host only."""

    @staticmethod
    def tables():
        """(exp (512,), log (256,)): exp[i] = 2^i with the cycle of 255 repeated, log[0] unused."""
        e, lg = np.zeros(512, np.uint8), np.zeros(256, np.uint8)
        _check(_L.orion_rs_gf_tables(e.ctypes.data, lg.ctypes.data))
        return e, lg

    @staticmethod
    def _u(a) -> int:
        a = int(a)
        if not 0 <= a <= 255:
            raise ValueError("gf: an element is 0..255")
        return a

    @staticmethod
    def add(a, b) -> int:
        return Gf256._u(a) ^ Gf256._u(b)

    @staticmethod
    def mul(a, b) -> int:
        return _gf_elem(_L.orion_rs_gf_mul(Gf256._u(a), Gf256._u(b)))

    @staticmethod
    def div(a, b) -> int:
        return _gf_elem(_L.orion_rs_gf_div(Gf256._u(a), Gf256._u(b)))

    @staticmethod
    def inv(a) -> int:
        return _gf_elem(_L.orion_rs_gf_inv(Gf256._u(a)))

    @staticmethod
    def pow(a, n) -> int:
        n = int(n)
        if n < 0:
            raise ValueError("gf pow: n >= 0")
        return _gf_elem(_L.orion_rs_gf_pow(Gf256._u(a), n if n < 1 << 63 else n % 255 + 255))

    @staticmethod
    def exp_of(i) -> int:
        i = int(i)
        if i < 0:
            raise ValueError("gf exp_of: i >= 0")
        return _gf_elem(_L.orion_rs_gf_exp_of(i % 255))


class RsUncorrectable(ValueError):
    """ReedSolomon.decode of an uncorrectable word; message is the systematic prefix received[:k]."""

    def __init__(self, message):
        super().__init__("codeword is uncorrectable")
        self.message = message


class ReedSolomon:
    """ReedSolomon (fec/reed_solomon.rs), host only: n codeword bytes, n_parity parity bytes
    (1 <= n <= 255, n_parity < n), t = n_parity // 2. Byte 0 is the highest-degree symbol."""

    def __init__(self, n, n_parity):
        n, n_parity = int(n), int(n_parity)
        if n < 1 or n > 255 or n_parity < 0 or n_parity >= n:
            raise ValueError("rs: code length n out of range 1..=255 or too short for the parity symbols")
        self.n, self.n_parity, self.k, self.t = n, n_parity, n - n_parity, n_parity // 2

    @classmethod
    def dvb(cls):
        """DVB-T's RS(204, 188), t = 8."""
        return cls(204, 16)

    @property
    def parity_bytes(self) -> int:
        return self.n_parity

    def generator(self) -> np.ndarray:
        """g(x) = prod (x - 2^i), i < n_parity, low degree first."""
        out = np.zeros(self.n_parity + 1, np.uint8)
        _arg_check(_L.orion_rs_generator(self.n, self.n_parity, out.ctypes.data))
        return out

    def _words(self, x, width, what):
        if isinstance(x, (bytes, bytearray)):
            x = np.frombuffer(bytes(x), np.uint8)
        if not isinstance(x, np.ndarray) or x.dtype != np.uint8 or x.ndim not in (1, 2) or x.shape[-1] != width:
            raise ValueError(f"{what}: expected uint8 ({width},) or (nwords, {width})")
        return np.ascontiguousarray(x), x.ndim == 1

    def encode(self, message) -> np.ndarray:
        """message (k,) or (nwords, k) -> codeword(s) message | parity."""
        m, one = self._words(message, self.k, "message")
        out = np.zeros(m.shape[:-1] + (self.n,), np.uint8)
        _arg_check(_L.orion_rs_encode(self.n, self.n_parity, m.ctypes.data, m.size // self.k, out.ctypes.data))
        return out

    def decode_counted(self, received):
        """decode_counted (reed_solomon.rs:141-233): received (n,) -> (message (k,), count),
        or (nwords, n) -> (messages (nwords, k), counts (nwords,) int32). count is the number of
        codeword bytes corrected, parity included; -1: uncorrectable, the message is then
        received[:k]."""
        r, one = self._words(received, self.n, "received")
        msgs = np.zeros(r.shape[:-1] + (self.k,), np.uint8)
        status = np.zeros(r.size // self.n, np.int32)
        _arg_check(_L.orion_rs_decode_counted(self.n, self.n_parity, r.ctypes.data, status.size, msgs.ctypes.data,
                                              status.ctypes.data))
        return (msgs, int(status[0])) if one else (msgs, status)

    def decode(self, received) -> np.ndarray:
        """decode (reed_solomon.rs:118-120) of one word; raises RsUncorrectable (carrying
        received[:k]) where the reference returns Uncorrectable."""
        r = _bytes_arg(received, "received")
        msg, count = self.decode_counted(r)
        if count < 0:
            raise RsUncorrectable(msg)
        return msg


def _forney_dims(branches, depth):
    branches, depth = int(branches), int(depth)
    if branches < 1 or depth < 1:
        raise ValueError("convolutional interleaver dimensions must be nonzero")
    if branches * branches * depth > 1 << 24:
        raise ValueError("convolutional interleaver: branches^2 * depth above 2^24")
    return branches, depth


class ConvInterleaver:
    """ConvInterleaver (fec/interleaver.rs:133-220), host only: the streaming Forney byte
    interleaver of `branches` branches, branch j a FIFO of j * depth bytes. feed is 1:1 in
    length and carries state across calls; flush feeds roundtrip_delay zeros; reset restarts."""

    _inverse = 0

    def __init__(self, branches, depth):
        self.branches, self.depth = _forney_dims(branches, depth)
        self._h = _L.orion_rs_forney_new(self.branches, self.depth, self._inverse)
        if not self._h:
            raise ValueError(_err())

    def __del__(self):
        if getattr(self, "_h", None):
            _L.orion_rs_forney_free(self._h)
            self._h = None

    @classmethod
    def dvb_t(cls):
        """DVB-T's outer interleaver: I = 12, M = 17."""
        return cls(12, 17)

    @property
    def roundtrip_delay(self) -> int:
        return self.branches * (self.branches - 1) * self.depth

    def reset(self):
        _check(_L.orion_rs_forney_reset(self._h))

    def feed(self, data) -> np.ndarray:
        d = _bytes_arg(data)
        out = np.zeros(d.size, np.uint8)
        _check(_L.orion_rs_forney_feed(self._h, d.ctypes.data, d.size, out.ctypes.data))
        return out

    def flush(self) -> np.ndarray:
        out = np.zeros(self.roundtrip_delay, np.uint8)
        _check(_L.orion_rs_forney_flush(self._h, out.ctypes.data))
        return out


class ConvDeinterleaver(ConvInterleaver):
    """ConvDeinterleaver (fec/interleaver.rs:226-305): the inverse, branch j a FIFO of
    (branches - 1 - j) * depth bytes; it reproduces the interleaver's input from output byte
    roundtrip_delay on."""

    _inverse = 1


def forney_frame_interleave(data, branches, depth) -> np.ndarray:
    """interleave_bits' Convolutional arm in bytes (modulate/ofdm_frame.rs:464-478), host only:
    data zero-padded to a multiple of branches bytes through a fresh interleaver, then the
    flush: round_up(n, branches) + branches (branches - 1) depth bytes."""
    branches, depth = _forney_dims(branches, depth)
    d = _bytes_arg(data)
    out = np.zeros(int(_L.orion_rs_forney_frame_len(branches, depth, d.size)), np.uint8)
    _arg_check(_L.orion_rs_forney_frame_interleave(branches, depth, d.ctypes.data, d.size, out.ctypes.data))
    return out


def forney_frame_deinterleave(data, branches, depth) -> np.ndarray:
    """deinterleave_bits' Convolutional arm in bytes (demodulate/ofdm_frame.rs:399-415), host
    only: data through a fresh deinterleaver, of which the bytes from the round-trip delay on
    are the padded payload (nothing when data is no longer than the delay)."""
    branches, depth = _forney_dims(branches, depth)
    d = _bytes_arg(data)
    out = np.zeros(max(d.size - branches * (branches - 1) * depth, 0), np.uint8)
    _arg_check(_L.orion_rs_forney_frame_deinterleave(branches, depth, d.ctypes.data, d.size, out.ctypes.data))
    return out


def _lfsr_args(taps, width, seed):
    taps, width, seed = int(taps), int(width), int(seed)
    if not 2 <= width <= 32:
        raise ValueError("LFSR width must be in 2..=32")
    mask = (1 << width) - 1
    if seed == 0:
        raise ValueError("LFSR seed must be nonzero")
    if seed < 0 or seed & ~mask or taps < 0 or taps & ~mask:
        raise ValueError("LFSR seed and taps must fit in `width` bits")
    return taps, width, seed


class PnScrambler:
    """PnScrambler (fec/scrambler.rs:39-104), host only: an additive Fibonacci LFSR whitener,
    data bits LSB first, restarted from seed on every scramble call (self-inverse)."""

    def __init__(self, taps, width, seed):
        self.taps, self.width, self.seed = _lfsr_args(taps, width, seed)

    def scramble(self, data) -> np.ndarray:
        out = _bytes_arg(data).copy()
        _arg_check(_L.orion_rs_pn_scramble(self.taps, self.width, self.seed, out.ctypes.data, out.size))
        return out

    def into_stream(self):
        return PnScramblerStream(self.taps, self.width, self.seed)


class PnScramblerStream:
    """PnScramblerStream (fec/scrambler.rs:133-195), host only: the same whitener with the
    register carried across feed calls; reset restarts from seed."""

    def __init__(self, taps, width, seed):
        self.taps, self.width, self.seed = _lfsr_args(taps, width, seed)
        self._h = _L.orion_rs_pn_stream_new(self.taps, self.width, self.seed)
        if not self._h:
            raise ValueError(_err())

    def __del__(self):
        if getattr(self, "_h", None):
            _L.orion_rs_pn_stream_free(self._h)
            self._h = None

    def reset(self):
        _check(_L.orion_rs_pn_stream_reset(self._h))

    def feed(self, data) -> np.ndarray:
        out = _bytes_arg(data).copy()
        _check(_L.orion_rs_pn_stream_feed(self._h, out.ctypes.data, out.size))
        return out


class DvbTEnergyDispersal:
    """DvbTEnergyDispersal (waveform/dvb_t.rs:30-110), host only: the PRBS 1 + X^14 + X^15 from
    100101010000000 XORed over the data MSB first, the register carried across feed calls;
    advance_byte clocks eight steps without output; reset reloads the init."""

    def __init__(self):
        self._h = _L.orion_rs_dispersal_new()
        if not self._h:
            raise OrionError(f"orion_sdr: construction failed: {_err()}")

    def __del__(self):
        if getattr(self, "_h", None):
            _L.orion_rs_dispersal_free(self._h)
            self._h = None

    def reset(self):
        _check(_L.orion_rs_dispersal_reset(self._h))

    def advance_byte(self):
        _check(_L.orion_rs_dispersal_advance_byte(self._h))

    def feed(self, data) -> np.ndarray:
        out = _bytes_arg(data).copy()
        _check(_L.orion_rs_dispersal_feed(self._h, out.ctypes.data, out.size))
        return out


def ts_energy_disperse(packets) -> np.ndarray:
    """ts_energy_disperse (waveform/dvb_t_ts.rs:53-79), host only, returning a copy: whole
    188-byte packets; the PRBS restarts every eight packets, the first sync byte of a group
    flips 0x47 <-> 0xB8, the others are clocked over, the payloads are whitened. Self-inverse."""
    out = _bytes_arg(packets, "packets").copy()
    _arg_check(_L.orion_rs_ts_energy_disperse(out.ctypes.data, out.size))
    return out


def ts_packetize(payload) -> np.ndarray:
    """ts_packetize (dvb_t_ts.rs:87-100): max(1, ceil(n / 187)) packets of 0x47 + 187 payload
    bytes, the last zero-padded."""
    p = _bytes_arg(payload, "payload")
    out = np.zeros(int(_L.orion_rs_ts_packetized_len(p.size)), np.uint8)
    _arg_check(_L.orion_rs_ts_packetize(p.ctypes.data, p.size, out.ctypes.data))
    return out


def ts_depacketize(packets):
    """ts_depacketize (dvb_t_ts.rs:139-148): the payloads of whole packets; None when packets
    is empty or no whole number of packets."""
    p = _bytes_arg(packets, "packets")
    if p.size == 0 or p.size % TS_PACKET_LEN:
        return None
    out = np.zeros(p.size // TS_PACKET_LEN * 187, np.uint8)
    _arg_check(_L.orion_rs_ts_depacketize(p.ctypes.data, p.size, out.ctypes.data))
    return out


def ts_null_packet() -> np.ndarray:
    """ts_null_packet (dvb_t_ts.rs:109-116): 47 1F FF 10 and 184 bytes of 0xFF."""
    out = np.zeros(TS_PACKET_LEN, np.uint8)
    _check(_L.orion_rs_ts_null_packet(out.ctypes.data))
    return out


def ts_stuff_null_packets(ts, target_packets) -> np.ndarray:
    """ts_stuff_null_packets (dvb_t_ts.rs:123-133), returning a copy: ts (whole packets)
    followed by null packets up to target_packets packets."""
    t = _bytes_arg(ts, "ts")
    target_packets = int(target_packets)
    if t.size % TS_PACKET_LEN or target_packets < 0 or target_packets > 1 << 32:
        raise ValueError("ts_stuff_null_packets: ts must be whole TS packets, 0 <= target_packets <= 2^32")
    out = np.zeros(max(t.size // TS_PACKET_LEN, target_packets) * TS_PACKET_LEN, np.uint8)
    _arg_check(_L.orion_rs_ts_stuff_null_packets(t.ctypes.data, t.size, target_packets, out.ctypes.data))
    return out


def _rs_u8(x, what, ndims):
    """x as a contiguous uint8 numpy array or torch CUDA tensor of one of ndims dimensions."""
    if _is_torch(x):
        import torch

        if not x.is_cuda or not x.is_contiguous() or x.dtype != torch.uint8 or x.dim() not in ndims:
            raise ValueError(f"{what}: a contiguous uint8 CUDA tensor of {' or '.join(map(str, ndims))} dimensions")
        return x, True
    if not isinstance(x, np.ndarray) or x.dtype != np.uint8 or x.ndim not in ndims:
        raise ValueError(f"{what}: expected a uint8 array of {' or '.join(map(str, ndims))} dimensions")
    return np.ascontiguousarray(x), False


def _rs_out(x, dev, shape, dtype):
    if dev:
        import torch

        return torch.empty(shape, dtype=getattr(torch, dtype), device=x.device)
    return np.zeros(shape, getattr(np, dtype))


def _rs_ptr(a, dev):
    return a.data_ptr() if dev else a.ctypes.data


def rs_encode_batch(msgs, n=204, n_parity=16, disperse=False, stream=None):
    """Reed-Solomon encode a batch on the GPU in one launch: uint8 (nstreams, ncw, k) or (ncw,
    k) -> (..., ncw, n), each word ReedSolomon(n, n_parity).encode of its message. disperse
    (k = 188): each stream's messages go through ts_energy_disperse first, word c of a stream
    being packet c. 1 <= n_parity <= 32. A numpy array (-> numpy) or a contiguous torch CUDA
    tensor (-> a torch tensor on its device, queued on torch's current stream or on stream)."""
    code = ReedSolomon(n, n_parity)
    m, dev = _rs_u8(msgs, "msgs", (2, 3))
    if m.shape[-1] != code.k:
        raise ValueError(f"msgs: the last dimension is k = {code.k}")
    ns, ncw = (1, int(m.shape[0])) if len(m.shape) == 2 else (int(m.shape[0]), int(m.shape[1]))
    out = _rs_out(m, dev, tuple(m.shape[:-1]) + (code.n,), "uint8")
    if dev:
        _arg_check(_L.orion_rs_encode_batch_device(code.n, code.n_parity, m.data_ptr(), ns, ncw, int(bool(disperse)),
                                                   out.data_ptr(), SyncEngine._stream(m, stream)))
    else:
        _arg_check(_L.orion_rs_encode_batch(code.n, code.n_parity, m.ctypes.data, ns, ncw, int(bool(disperse)),
                                            out.ctypes.data))
    return out


def rs_decode_batch(x, n=204, n_parity=16, bits=False, deinterleave=None, derandomize=False, stream=None):
    """Reed-Solomon decode a batch on the GPU in one launch, one wave per codeword: returns
    (msgs, status), status int32 the corrected-byte count of each word or -1 for an
    uncorrectable one (whose message is received[:k]); both equal
    ReedSolomon(n, n_parity).decode_counted of every word. 1 <= n_parity <= 32.

    Without bits and deinterleave, x is uint8 (nstreams, ncw, n) or (ncw, n) and msgs (...,
    ncw, k), status (..., ncw). Otherwise x is one flat stream per row, (nstreams, len) or
    (len,), and msgs is (nstreams, ncw, k) or (ncw, k): bits: every byte as eight elements of
    one bit, MSB first (the tensor conv_viterbi_batch returns is taken as it is); deinterleave
    = (branches, depth): the stream is forney_frame_interleave of the ncw * n codeword bytes
    (a multiple of branches), undone in the fetch. derandomize (k = 188): the messages go
    through ts_energy_disperse per stream, failed words included. A numpy array (-> numpy) or
    a contiguous torch CUDA tensor (-> torch tensors on its device, queued on torch's current
    stream or on stream)."""
    code = ReedSolomon(n, n_parity)
    I, M = _forney_dims(*deinterleave) if deinterleave is not None else (0, 0)
    flat = bool(bits) or I > 0
    a, dev = _rs_u8(x, "x", (1, 2) if flat else (2, 3))
    if flat:
        batched = len(a.shape) == 2
        ns, length = (int(a.shape[0]), int(a.shape[1])) if batched else (1, int(a.shape[0]))
        unit = 8 if bits else 1
        payload = length // unit - I * (I - 1) * M
        if length % unit or payload < code.n or payload % code.n:
            raise ValueError("x: a stream is ncw * n bytes, plus the interleaver's round-trip delay, times 8 for bits")
        ncw = payload // code.n
        lead = (ns, ncw) if batched else (ncw,)
    else:
        if a.shape[-1] != code.n:
            raise ValueError(f"x: the last dimension is n = {code.n}")
        ns, ncw = (1, int(a.shape[0])) if len(a.shape) == 2 else (int(a.shape[0]), int(a.shape[1]))
        lead = tuple(a.shape[:-1])
    if ncw < 1:
        raise ValueError("x: at least one codeword per stream")
    msgs, status = _rs_out(a, dev, lead + (code.k,), "uint8"), _rs_out(a, dev, lead, "int32")
    args = (code.n, code.n_parity, _rs_ptr(a, dev), ns, ncw, int(bool(bits)), I, M, int(bool(derandomize)),
            _rs_ptr(msgs, dev), _rs_ptr(status, dev))
    if dev:
        _arg_check(_L.orion_rs_decode_batch_device(*args, SyncEngine._stream(a, stream)))
    else:
        _arg_check(_L.orion_rs_decode_batch(*args))
    return msgs, status


def forney_interleave_batch(x, branches, depth, bits=False, stream=None):
    """The frame-mode Forney interleaver of a batch on the GPU in one launch: uint8 (nstreams,
    len), (len,) or (nstreams, ncw, n) (a stream is then its ncw * n bytes) -> (nstreams, out)
    or (out,), each row forney_frame_interleave of its stream; bits: unpacked to one bit per
    element, MSB first, which conv_encode_batch takes as it is. A numpy array (-> numpy) or a
    contiguous torch CUDA tensor (-> a torch tensor on its device, queued on torch's current
    stream or on stream)."""
    I, M = _forney_dims(branches, depth)
    a, dev = _rs_u8(x, "x", (1, 2, 3))
    batched = len(a.shape) > 1
    ns = int(a.shape[0]) if batched else 1
    length = 1
    for d in a.shape[1 if batched else 0:]:
        length *= int(d)
    out_len = int(_L.orion_rs_forney_interleave_len(I, M, length, int(bool(bits))))
    if out_len == 0:
        raise ValueError(_err())
    out = _rs_out(a, dev, (ns, out_len) if batched else (out_len,), "uint8")
    if dev:
        _arg_check(_L.orion_rs_forney_interleave_batch_device(I, M, a.data_ptr(), ns, length, int(bool(bits)),
                                                              out.data_ptr(), SyncEngine._stream(a, stream)))
    else:
        _arg_check(_L.orion_rs_forney_interleave_batch(I, M, a.ctypes.data, ns, length, int(bool(bits)),
                                                       out.ctypes.data))
    return out


# ---- the frame chain's codes: the constructed LDPC family and the shortened BCH code
# (src/fec/ldpc_codes.rs, src/fec/bch.rs) ----
def _fec2_sigs():
    vp, sz, i, f = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    sig = {
        "orion_ldpcf_dims": (i, [i, vp]), "orion_ldpcf_graph": (i, [i, vp, vp, vp, vp, vp]),
        "orion_ldpcf_encode": (i, [i, vp, sz, vp]), "orion_ldpcf_syndrome_weight": (i, [i, vp, sz, vp]),
        "orion_ldpcf_decode_soft": (i, [i, vp, sz, sz, i, f, vp, vp, vp]),
        "orion_ldpcf_decode_blocks": (sz, [i, sz, sz, sz]),
        "orion_ldpcf_decode_batch": (i, [i, vp, sz, sz, sz, sz, sz, i, f, vp, vp, vp]),
        "orion_ldpcf_decode_batch_device": (i, [i, vp, sz, sz, sz, sz, sz, i, f, vp, vp, vp, vp]),
        "orion_ldpcf_encoded_len": (sz, [i, sz, sz, sz]),
        "orion_ldpcf_encode_batch": (i, [i, vp, sz, sz, sz, sz, vp]),
        "orion_ldpcf_encode_batch_device": (i, [i, vp, sz, sz, sz, sz, vp, vp]),
        "orion_bch_parity_bits": (sz, [sz]), "orion_bch_generator": (i, [sz, sz, vp]),
        "orion_bch_encode": (i, [sz, sz, vp, sz, vp]), "orion_bch_decode": (i, [sz, sz, vp, sz, vp, vp, vp]),
        "orion_bch_decode_batch": (i, [sz, sz, vp, sz, sz, vp, vp]),
        "orion_bch_decode_batch_device": (i, [sz, sz, vp, sz, sz, vp, vp, vp]),
        "orion_bch_encode_batch": (i, [sz, sz, vp, sz, sz, vp]),
        "orion_bch_encode_batch_device": (i, [sz, sz, vp, sz, sz, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(_L, name)
        fn.restype = res
        fn.argtypes = args


_fec2_sigs()

LDPC_CODES = {"n512r12": 0, "n576r23": 1, "n512r34": 2}  # ldpc_codes.rs:46-73
LDPC_RULES = {"sum_product": 0, "min_sum": 1, "scaled_min_sum": 2}  # ldpc_codes.rs:97-105
BCH_INFO_BITS = 120  # modulate/ofdm_frame.rs:485
__all__ += ["LDPC_CODES", "LDPC_RULES", "BCH_INFO_BITS", "Ldpc", "Bch", "BchUncorrectable", "ldpc_family_encode_batch",
            "ldpc_family_decode_batch", "bch_encode_batch", "bch_decode_batch"]


def _ldpcf_code(code) -> int:
    if isinstance(code, Ldpc):
        return code.index
    if not isinstance(code, str) or code not in LDPC_CODES:
        raise ValueError(f"code: one of {sorted(LDPC_CODES)}")
    return LDPC_CODES[code]


def _ldpcf_rule(rule):
    """"sum_product", "min_sum" or ("scaled_min_sum", a) -> (rule index, scale)."""
    if isinstance(rule, str) and rule in ("sum_product", "min_sum"):
        return LDPC_RULES[rule], 1.0
    if isinstance(rule, (tuple, list)) and len(rule) == 2 and rule[0] == "scaled_min_sum":
        try:
            return LDPC_RULES["scaled_min_sum"], float(np.float32(rule[1]))
        except (TypeError, ValueError):
            pass
    raise ValueError('rule: "sum_product", "min_sum" or ("scaled_min_sum", a)')


def _ldpcf_max_iter(max_iter) -> int:
    max_iter = int(max_iter)
    if max_iter < 0 or max_iter > 1 << 30:
        raise ValueError("max_iter: 0 to 2^30")
    return max_iter


class Ldpc:
    """Ldpc (fec/ldpc_codes.rs), host only: one of the three constructed codes "n512r12" (N =
    512, K = 256), "n576r23" (576, 384), "n512r34" (512, 384). The library builds a code on
    first use and keeps it. LLRs are positive for bit 0."""

    def __init__(self, code):
        self.index = _ldpcf_code(code)
        self.code = code.code if isinstance(code, Ldpc) else code
        d = np.zeros(6, np.uint32)
        _arg_check(_L.orion_ldpcf_dims(self.index, d.ctypes.data))
        self.n, self.k, self.m, self.n_edges, self.max_check_degree, self.relaxed_picks = (int(v) for v in d)

    def graph(self):
        """The Tanner graph as CSR, uint32: check_start (M + 1,), check_bits (edges,) (within a
        check the message columns ascending, then K + i, then K + i - 1), bit_start (N + 1,),
        bit_checks (edges,) (ascending) and bit_edges (edges,), the index into check_bits of
        that bit in that check."""
        g = {"check_start": np.zeros(self.m + 1, np.uint32), "check_bits": np.zeros(self.n_edges, np.uint32),
             "bit_start": np.zeros(self.n + 1, np.uint32), "bit_checks": np.zeros(self.n_edges, np.uint32),
             "bit_edges": np.zeros(self.n_edges, np.uint32)}
        _arg_check(_L.orion_ldpcf_graph(self.index, *(a.ctypes.data for a in g.values())))
        return g

    @staticmethod
    def _words(x, width, dtype, what):
        if not isinstance(x, np.ndarray) or x.dtype != dtype or x.ndim not in (1, 2) or x.shape[-1] != width:
            raise ValueError(f"{what}: expected {np.dtype(dtype).name} ({width},) or (nwords, {width})")
        return np.ascontiguousarray(x), x.ndim == 1

    def encode(self, message) -> np.ndarray:
        """message (K,) or (nwords, K) uint8 -> codeword(s) message | parity (N)."""
        m, _ = self._words(message, self.k, np.uint8, "message")
        out = np.zeros(m.shape[:-1] + (self.n,), np.uint8)
        _arg_check(_L.orion_ldpcf_encode(self.index, m.ctypes.data, m.size // self.k, out.ctypes.data))
        return out

    def syndrome_weight(self, hard):
        """Unsatisfied checks of hard (N,) -> int, or (nwords, N) -> int32 (nwords,)."""
        h, one = self._words(hard, self.n, np.uint8, "hard")
        out = np.zeros(h.size // self.n, np.int32)
        _arg_check(_L.orion_ldpcf_syndrome_weight(self.index, h.ctypes.data, out.size, out.ctypes.data))
        return int(out[0]) if one else out

    def decode_soft(self, llr, max_iter=50, rule="sum_product"):
        """decode_soft_with (ldpc_codes.rs:366-540): float32 llr (N,) -> (bits (K,), unsat,
        iterations), or (nwords, N) -> (bits (nwords, K), unsat, iterations int32 (nwords,)).
        unsat is the smallest unsatisfied-check count seen (0: decoded), iterations the
        iterations run (0: the initial decision was a codeword). rule: "sum_product",
        "min_sum" or ("scaled_min_sum", a)."""
        r, scale = _ldpcf_rule(rule)
        l, one = self._words(llr, self.n, np.float32, "llr")
        nw = l.size // self.n
        bits = np.zeros(l.shape[:-1] + (self.k,), np.uint8)
        unsat, iters = np.zeros(nw, np.int32), np.zeros(nw, np.int32)
        _arg_check(_L.orion_ldpcf_decode_soft(self.index, l.ctypes.data, nw, _ldpcf_max_iter(max_iter), r, scale,
                                              bits.ctypes.data, unsat.ctypes.data, iters.ctypes.data))
        return (bits, int(unsat[0]), int(iters[0])) if one else (bits, unsat, iters)


class BchUncorrectable(ValueError):
    """Bch.decode of an uncorrectable word; message is the systematic prefix received[:k],
    errors the reference's payload max(residual syndromes, roots found)."""

    def __init__(self, message, errors):
        super().__init__(f"codeword has {errors} residual errors after decoding (uncorrectable)")
        self.message = message
        self.errors = errors


class Bch:
    """Bch (fec/bch.rs), host only: the binary BCH code over GF(2^8) correcting t bit errors,
    shortened to n elements (1 <= n <= 255, parity bits < n) of one bit each, index 0 the
    highest degree. An element is set when it is nonzero; a correction is ^= 1."""

    def __init__(self, t, n=255):
        t, n = int(t), int(n)
        if t < 1:
            raise ValueError("bch: design t = 0")
        pb = int(_L.orion_bch_parity_bits(t)) if t <= 1 << 16 else 0
        if pb == 0:
            raise ValueError("bch: design t is too large for GF(2^8) (parity would exceed the block)")
        if n < 1 or n > 255 or pb >= n:
            raise ValueError("bch: shortened length n is out of range 1..=255 or leaves no room for parity")
        self.t, self.n, self.parity_bits, self.k = t, n, pb, n - pb

    @classmethod
    def for_info_bits(cls, t, info_bits=BCH_INFO_BITS):
        """shortened_bch_for (modulate/ofdm_frame.rs:547-552): the code of t whose message is
        info_bits long; the frame's is t = 8 over 120 bits, n = 184."""
        info_bits = int(info_bits)
        if info_bits < 1:
            raise ValueError("info_bits: at least 1")
        return cls(t, info_bits + cls(t).parity_bits)

    def generator(self) -> np.ndarray:
        """g(x), highest degree first, 0 / 1: parity_bits + 1 coefficients."""
        out = np.zeros(self.parity_bits + 1, np.uint8)
        _arg_check(_L.orion_bch_generator(self.n, self.t, out.ctypes.data))
        return out

    def _words(self, x, width, what):
        if not isinstance(x, np.ndarray) or x.dtype != np.uint8 or x.ndim not in (1, 2) or x.shape[-1] != width:
            raise ValueError(f"{what}: expected uint8 ({width},) or (nwords, {width})")
        return np.ascontiguousarray(x), x.ndim == 1

    def encode(self, message) -> np.ndarray:
        """message (k,) or (nwords, k) -> codeword(s) message | parity."""
        m, _ = self._words(message, self.k, "message")
        out = np.zeros(m.shape[:-1] + (self.n,), np.uint8)
        _arg_check(_L.orion_bch_encode(self.n, self.t, m.ctypes.data, m.size // self.k, out.ctypes.data))
        return out

    def decode_counted(self, received, locator_len=False):
        """decode (bch.rs:131-207) with its outcome as a number: received (n,) -> (message (k,),
        status), or (nwords, n) -> (messages (nwords, k), status int32 (nwords,)). status is the
        number of bits flipped, parity included, or -max(residual syndromes, roots found) <= -1
        for an uncorrectable word, whose message is received[:k]. locator_len: also the
        entries of the Berlekamp-Massey locator vector (0 for a clean word)."""
        r, one = self._words(received, self.n, "received")
        msgs = np.zeros(r.shape[:-1] + (self.k,), np.uint8)
        status, loc = np.zeros(r.size // self.n, np.int32), np.zeros(r.size // self.n, np.int32)
        _arg_check(_L.orion_bch_decode(self.n, self.t, r.ctypes.data, status.size, msgs.ctypes.data, status.ctypes.data,
                                       loc.ctypes.data))
        out = (msgs, int(status[0])) if one else (msgs, status)
        return out + ((int(loc[0]) if one else loc),) if locator_len else out

    def decode(self, received) -> np.ndarray:
        """decode of one word; raises BchUncorrectable (carrying received[:k]) where the
        reference returns Uncorrectable."""
        if not isinstance(received, np.ndarray) or received.ndim != 1:
            raise ValueError(f"received: expected uint8 ({self.n},)")
        msg, status = self.decode_counted(received)
        if status < 0:
            raise BchUncorrectable(msg, -status)
        return msg


def _fec2_arg(x, what, dtype, ndims):
    """x as a contiguous numpy array or torch CUDA tensor of dtype and one of ndims dimensions."""
    if _is_torch(x):
        import torch

        if not x.is_cuda or not x.is_contiguous() or x.dtype != getattr(torch, dtype) or x.dim() not in ndims:
            raise ValueError(f"{what}: a contiguous {dtype} CUDA tensor of {' or '.join(map(str, ndims))} dimensions")
        return x, True
    if not isinstance(x, np.ndarray) or x.dtype != getattr(np, dtype) or x.ndim not in ndims:
        raise ValueError(f"{what}: expected a {dtype} array of {' or '.join(map(str, ndims))} dimensions")
    return np.ascontiguousarray(x), False


def ldpc_family_encode_batch(bits, code, interleaver=None, stream=None):
    """LDPC encode and (with interleaver, a BlockInterleaver or (rows, cols)) block interleave a
    batch of streams on the GPU in one launch: uint8 (nstreams, nbits) -> uint8 (nstreams, coded
    length): ceil(nbits / K) codewords of code ("n512r12", "n576r23", "n512r34"), the last
    message zero-padded, rounded up to whole interleaver blocks (zero padding). Row k is
    interleave_bits of the Ldpc(code).encode of its K-bit blocks. A numpy array (-> numpy) or a
    contiguous torch CUDA tensor (-> a torch tensor on its device, queued on torch's current
    stream or on stream)."""
    c = _ldpcf_code(code)
    rows, cols = _fec_il(interleaver)
    b, dev = _fec2_arg(bits, "bits", "uint8", (2,))
    ns, nbits = int(b.shape[0]), int(b.shape[1])
    if nbits < 1:
        raise ValueError("bits: at least one bit per stream")
    out_len = int(_L.orion_ldpcf_encoded_len(c, nbits, rows, cols))
    if out_len == 0:
        raise ValueError(_err())
    out = _rs_out(b, dev, (ns, out_len), "uint8")
    if dev:
        _arg_check(_L.orion_ldpcf_encode_batch_device(c, b.data_ptr(), ns, nbits, rows, cols, out.data_ptr(),
                                                      SyncEngine._stream(b, stream)))
    else:
        _arg_check(_L.orion_ldpcf_encode_batch(c, b.ctypes.data, ns, nbits, rows, cols, out.ctypes.data))
    return out


def ldpc_family_decode_batch(llr, code, max_iter=50, rule="sum_product", interleaver=None, stream=None):
    """Belief-propagation decode of a batch of streams on the GPU in one launch, one wave per
    codeword, the block deinterleaver fused into the LLR fetch: float32 (nstreams, n_llr),
    positive meaning bit 0 -> (bits uint8 (nstreams, nblocks * K), unsat int32 (nstreams,
    nblocks), iterations int32 (nstreams, nblocks)), nblocks = n_llr // N. Codeword LLR j of a
    stream is element j of deinterleave_llrs(llr[k]) (n_llr must then be whole interleaver
    blocks); what lies past nblocks * N is padding and is not read. Every word equals
    Ldpc(code).decode_soft(word, max_iter, rule) in all three outputs. rule: "sum_product",
    "min_sum" or ("scaled_min_sum", a). A numpy array (-> numpy) or a contiguous torch CUDA
    tensor, such as the llr of ofdm_demodulate_batch(..., llr=True) (-> torch tensors on its
    device, queued on torch's current stream or on stream)."""
    c = _ldpcf_code(code)
    r, scale = _ldpcf_rule(rule)
    mi = _ldpcf_max_iter(max_iter)
    rows, cols = _fec_il(interleaver)
    l, dev = _fec2_arg(llr, "llr", "float32", (2,))
    ns, nl = int(l.shape[0]), int(l.shape[1])
    nblocks = int(_L.orion_ldpcf_decode_blocks(c, nl, rows, cols))
    if nblocks == 0:
        raise ValueError(_err())
    k = (256, 384, 384)[c]
    bits, unsat, iters = (_rs_out(l, dev, (ns, nblocks * k), "uint8"), _rs_out(l, dev, (ns, nblocks), "int32"),
                          _rs_out(l, dev, (ns, nblocks), "int32"))
    args = (c, _rs_ptr(l, dev), ns, nl, rows, cols, mi, r, scale, _rs_ptr(bits, dev), _rs_ptr(unsat, dev),
            _rs_ptr(iters, dev))
    if dev:
        _arg_check(_L.orion_ldpcf_decode_batch_device(*args, SyncEngine._stream(l, stream)))
    else:
        _arg_check(_L.orion_ldpcf_decode_batch(*args))
    return bits, unsat, iters


def _bch_device_code(t, info_bits):
    t = int(t)
    if t < 1 or t > 31:
        raise ValueError("bch: 1 <= t <= 31 on the device")
    return Bch.for_info_bits(t, info_bits)


def bch_encode_batch(bits, t, info_bits=BCH_INFO_BITS, stream=None):
    """BCH encode a batch of streams on the GPU in one launch, one wave per word: uint8
    (nstreams, nbits) or (nbits,) -> (..., ncw * n), ncw = ceil(nbits / info_bits) words of
    Bch.for_info_bits(t, info_bits), the last message zero-padded (outer_encode,
    modulate/ofdm_frame.rs:495-505). 1 <= t <= 31. A numpy array (-> numpy) or a contiguous
    torch CUDA tensor (-> a torch tensor on its device, queued on torch's current stream or on
    stream)."""
    code = _bch_device_code(t, info_bits)
    b, dev = _fec2_arg(bits, "bits", "uint8", (1, 2))
    batched = len(b.shape) == 2
    ns, nbits = (int(b.shape[0]), int(b.shape[1])) if batched else (1, int(b.shape[0]))
    if nbits < 1:
        raise ValueError("bits: at least one bit per stream")
    out_len = -(-nbits // code.k) * code.n
    out = _rs_out(b, dev, (ns, out_len) if batched else (out_len,), "uint8")
    if dev:
        _arg_check(_L.orion_bch_encode_batch_device(code.t, code.k, b.data_ptr(), ns, nbits, out.data_ptr(),
                                                    SyncEngine._stream(b, stream)))
    else:
        _arg_check(_L.orion_bch_encode_batch(code.t, code.k, b.ctypes.data, ns, nbits, out.ctypes.data))
    return out


def bch_decode_batch(bits, t, info_bits=BCH_INFO_BITS, stream=None):
    """BCH decode a batch of streams on the GPU in one launch, one wave per word: uint8
    (nstreams, nb) or (nb,), one bit per element as ldpc_family_decode_batch or
    conv_viterbi_batch write them -> (bits (..., ncw * info_bits), status int32 (..., ncw)), ncw
    = nb // n words of Bch.for_info_bits(t, info_bits) per stream, the tail ignored. Both equal
    Bch.decode_counted of every word: status is the number of bits flipped, or negative for an
    uncorrectable word, whose message is received[:k]. 1 <= t <= 31. A numpy array (-> numpy)
    or a contiguous torch CUDA tensor (-> torch tensors on its device, queued on torch's
    current stream or on stream)."""
    code = _bch_device_code(t, info_bits)
    b, dev = _fec2_arg(bits, "bits", "uint8", (1, 2))
    batched = len(b.shape) == 2
    ns, nb = (int(b.shape[0]), int(b.shape[1])) if batched else (1, int(b.shape[0]))
    ncw = nb // code.n
    if ncw < 1:
        raise ValueError(f"bits: a stream is at least one codeword of n = {code.n} bits")
    msgs = _rs_out(b, dev, (ns, ncw * code.k) if batched else (ncw * code.k,), "uint8")
    status = _rs_out(b, dev, (ns, ncw) if batched else (ncw,), "int32")
    args = (code.t, code.k, _rs_ptr(b, dev), ns, nb, _rs_ptr(msgs, dev), _rs_ptr(status, dev))
    if dev:
        _arg_check(_L.orion_bch_decode_batch_device(*args, SyncEngine._stream(b, stream)))
    else:
        _arg_check(_L.orion_bch_decode_batch(*args))
    return msgs, status


# ---- the COFDM frame layer's coding chain: CRCs, header fields, scramblers, the block plan,
# encode_chain / decode_chain and the kernels between the batched codes
# (src/modulate/ofdm_frame.rs:204-682, src/demodulate/ofdm_frame.rs:351-779, src/codec/crc.rs:89-130,
# src/fec/frame.rs) ----
class _FrameSchemeC(C.Structure):
    _fields_ = [("crc", C.c_int32), ("outer", C.c_int32), ("outer_a", C.c_uint32), ("outer_b", C.c_uint32),
                ("inner", C.c_int32), ("inner_a", C.c_uint32), ("inner_b", C.c_uint32),
                ("outer_il", C.c_int32), ("outer_il_a", C.c_uint32), ("outer_il_b", C.c_uint32),
                ("inner_il", C.c_int32), ("inner_il_a", C.c_uint32), ("inner_il_b", C.c_uint32),
                ("scrambler", C.c_int32), ("scr_poly", C.c_uint32), ("scr_width", C.c_uint32),
                ("scr_per_frame", C.c_int32), ("scr_seed", C.c_uint32), ("scrambler_pos", C.c_int32)]


def _frame_sigs():
    vp, sz, i, f, u = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_uint32
    sp = C.POINTER(_FrameSchemeC)
    sig = {
        "orion_frame_crc16": (u, [vp, sz]), "orion_frame_crc32": (u, [vp, sz]),
        "orion_frame_append_crc": (i, [i, vp, sz, vp]), "orion_frame_check_crc": (i, [i, vp, sz, vp]),
        "orion_frame_pack_header": (i, [vp, vp]), "orion_frame_unpack_header": (i, [vp, vp]),
        "orion_frame_reduce_seed": (u, [u, u]),
        "orion_frame_scramble_bytes": (i, [sp, u, vp, sz]), "orion_frame_scramble_bits": (i, [sp, u, vp, sz]),
        "orion_frame_apply_pn_to_llrs": (i, [sp, u, vp, sz]), "orion_frame_block_plan": (i, [sp, sz, vp]),
        "orion_frame_encode_chain": (i, [sp, vp, sz, u, vp, vp]),
        "orion_frame_decode_chain": (i, [sp, vp, sz, sz, u, i, f, vp, vp, vp, sz, vp]),
        "orion_frame_pack_batch": (i, [sp, vp, vp, vp, sz, sz, i, vp]),
        "orion_frame_pack_batch_device": (i, [sp, vp, vp, vp, sz, sz, i, vp, vp]),
        "orion_frame_unpack_batch": (i, [sp, vp, sz, i, vp, vp, sz, vp, sz, sz, sz, vp, vp, vp, vp]),
        "orion_frame_unpack_batch_device": (i, [sp, vp, sz, i, vp, vp, sz, vp, sz, sz, sz, vp, vp, vp, vp, vp]),
        "orion_frame_coded_bits_batch": (i, [sp, vp, sz, sz, vp, sz, sz, vp]),
        "orion_frame_coded_bits_batch_device": (i, [sp, vp, sz, sz, vp, sz, sz, vp, vp]),
        "orion_frame_llr_prepare_batch": (i, [sp, vp, sz, sz, vp, sz, vp]),
        "orion_frame_llr_prepare_batch_device": (i, [sp, vp, sz, sz, vp, sz, vp, vp]),
        "orion_frame_bytes_to_bits_batch": (i, [vp, sz, sz, vp]),
        "orion_frame_bytes_to_bits_batch_device": (i, [vp, sz, sz, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(_L, name)
        fn.restype = res
        fn.argtypes = args


_frame_sigs()

CRC_KINDS = {"none": 0, "crc16": 1, "crc32": 2}  # fec/frame.rs:131-151
HEADER_FIELD_BYTES = 14  # modulate/ofdm_frame.rs:128
# RxError (fec/frame.rs:59-77) as the codes the frame calls report; 0 is no error
RX_ERRORS = {"preamble_timeout": 1, "malformed_header": 2, "header_crc_mismatch": 3, "crc_mismatch": 4,
             "fec_uncorrectable": 5}
__all__ += ["CRC_KINDS", "HEADER_FIELD_BYTES", "RX_ERRORS", "FrameScheme", "BlockPlan", "ChainOutcome", "crc16",
            "crc32", "append_crc", "check_and_strip_crc", "bytes_to_bits", "bits_to_bytes", "pack_header_fields",
            "unpack_header_fields", "scrambler_seed", "scramble_bytes", "scramble_bits", "apply_pn_to_llrs",
            "block_plan", "symbols_for_coded_bits", "encode_chain", "encode_chain_stages", "decode_chain",
            "frame_pack_batch", "frame_unpack_batch", "frame_coded_bits_batch", "frame_llr_prepare_batch",
            "frame_bytes_to_bits_batch", "frame_encode_chain_batch", "frame_decode_chain_batch"]


class RxError(Exception):
    """RxError (fec/frame.rs:59-77): why a received frame could not be delivered. code is the
    RX_ERRORS value, kind its name."""

    def __init__(self, code):
        code = RX_ERRORS[code] if isinstance(code, str) else int(code)
        self.code = code
        self.kind = {v: k for k, v in RX_ERRORS.items()}.get(code, "unknown")
        super().__init__(self.kind)

    def __eq__(self, other):
        return isinstance(other, RxError) and other.code == self.code

    def __hash__(self):
        return hash(self.code)


def _u32(v, what) -> int:
    v = int(v)
    if v < 0 or v > 0xFFFFFFFF:
        raise ValueError(f"{what}: 0 .. 2^32 - 1")
    return v


class FrameScheme:
    """One logical block's coding chain, encode_chain's arguments after the bytes
    (modulate/ofdm_frame.rs:621-632):

    crc "none" / "crc16" / "crc32"; outer None, ("bch", t) or ("rs", n, n_parity); inner None,
    ("ldpc", code) or ("conv", rate[, code]); outer_interleaver / inner_interleaver None, ("block",
    rows, cols) or ("forney", branches, depth); scrambler None, "dvbt" or ("additive", poly, width,
    seed) with seed an int (SeedMode::Fixed) or "per_frame" (the seed then comes with each call
    or frame); scrambler_pos "before_outer" / "after_inner"."""

    def __init__(self, crc="crc32", outer=None, inner=None, outer_interleaver=None, inner_interleaver=None,
                 scrambler=None, scrambler_pos="before_outer"):
        c = _FrameSchemeC()
        if crc not in CRC_KINDS:
            raise ValueError(f"crc: one of {sorted(CRC_KINDS)}")
        c.crc = CRC_KINDS[crc]
        if outer is not None:
            if outer[0] == "bch" and len(outer) == 2:
                c.outer, c.outer_a = 1, _u32(outer[1], "t")
            elif outer[0] in ("rs", "reed_solomon") and len(outer) == 3:
                c.outer, c.outer_a, c.outer_b = 2, _u32(outer[1], "n"), _u32(outer[2], "n_parity")
            else:
                raise ValueError('outer: None, ("bch", t) or ("rs", n, n_parity)')
        if inner is not None:
            if inner[0] == "ldpc" and len(inner) == 2:
                c.inner, c.inner_a = 1, _ldpcf_code(inner[1])
            elif inner[0] in ("conv", "convolutional") and len(inner) in (2, 3):
                c.inner, c.inner_b = 2, _fec_rate(inner[1])
                c.inner_a = _fec_code(inner[2] if len(inner) == 3 else "k5")
            else:
                raise ValueError('inner: None, ("ldpc", code) or ("conv", rate[, code])')
        for name, il in (("outer_il", outer_interleaver), ("inner_il", inner_interleaver)):
            if il is None:
                continue
            if len(il) != 3 or il[0] not in ("block", "forney", "convolutional"):
                raise ValueError('interleaver: None, ("block", rows, cols) or ("forney", branches, depth)')
            setattr(c, name, 1 if il[0] == "block" else 2)
            setattr(c, name + "_a", _u32(il[1], "interleaver"))
            setattr(c, name + "_b", _u32(il[2], "interleaver"))
        if scrambler is not None:
            if scrambler in ("dvbt", "dvb_t"):
                c.scrambler = 2
            elif not isinstance(scrambler, str) and len(scrambler) == 4 and scrambler[0] == "additive":
                c.scrambler, c.scr_poly, c.scr_width = 1, _u32(scrambler[1], "poly"), _u32(scrambler[2], "width")
                if scrambler[3] == "per_frame":
                    c.scr_per_frame = 1
                else:
                    c.scr_seed = _u32(scrambler[3], "seed")
            else:
                raise ValueError('scrambler: None, "dvbt" or ("additive", poly, width, seed | "per_frame")')
        if scrambler_pos not in ("before_outer", "after_inner"):
            raise ValueError('scrambler_pos: "before_outer" or "after_inner"')
        c.scrambler_pos = 0 if scrambler_pos == "before_outer" else 1
        self._c = c
        self.crc, self.outer, self.inner = crc, outer, inner
        self.outer_interleaver, self.inner_interleaver = outer_interleaver, inner_interleaver
        self.scrambler, self.scrambler_pos = scrambler, scrambler_pos
        block_plan(0, self)  # the library's check of every parameter

    @property
    def crc_len(self) -> int:
        return (0, 2, 4)[self._c.crc]

    @property
    def per_frame_seed(self) -> bool:
        return bool(self._c.scr_per_frame)

    def _ptr(self):
        return C.byref(self._c)


def _frame_scheme(scheme) -> FrameScheme:
    if not isinstance(scheme, FrameScheme):
        raise ValueError("scheme: a FrameScheme")
    return scheme


def crc16(data) -> int:
    """CRC-16/CCITT-FALSE (codec/crc.rs:94-108): crc16(b"123456789") == 0x29B1."""
    b = _bytes_arg(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data)
    return int(_L.orion_frame_crc16(b.ctypes.data, b.size))


def crc32(data) -> int:
    """CRC-32/ISO-HDLC (codec/crc.rs:116-130): crc32(b"123456789") == 0xCBF43926."""
    b = _bytes_arg(np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else data)
    return int(_L.orion_frame_crc32(b.ctypes.data, b.size))


def _crc_kind(crc) -> int:
    if crc not in CRC_KINDS:
        raise ValueError(f"crc: one of {sorted(CRC_KINDS)}")
    return CRC_KINDS[crc]


def append_crc(crc, data) -> np.ndarray:
    """append_crc (modulate/ofdm_frame.rs:237-245): data | its CRC, big-endian."""
    k, b = _crc_kind(crc), _bytes_arg(data)
    out = np.zeros(b.size + (0, 2, 4)[k], np.uint8)
    _arg_check(_L.orion_frame_append_crc(k, b.ctypes.data, b.size, out.ctypes.data))
    return out


def check_and_strip_crc(crc, data):
    """check_and_strip_crc (modulate/ofdm_frame.rs:249-261): (payload, crc_ok), or None when data
    is shorter than the CRC field."""
    k, b = _crc_kind(crc), _bytes_arg(data)
    clen = (0, 2, 4)[k]
    if b.size < clen:
        return None
    ok = C.c_int32(0)
    _arg_check(_L.orion_frame_check_crc(k, b.ctypes.data, b.size, C.byref(ok)))
    return b[:b.size - clen].copy(), bool(ok.value)


def bytes_to_bits(data) -> np.ndarray:
    """bytes_to_bits (modulate/ofdm_frame.rs:207-215): MSB first, one bit per element."""
    return np.unpackbits(_bytes_arg(data))


def bits_to_bytes(bits) -> np.ndarray:
    """bits_to_bytes (modulate/ofdm_frame.rs:219-234): bit 0 of each element, MSB first; the
    count must be a whole number of bytes."""
    b = _bytes_arg(bits, "bits")
    if b.size % 8:
        raise ValueError("bit count must be a whole number of bytes")
    return np.packbits(b & 1)


def pack_header_fields(mcs_index, payload_len, sequence_num, flags, scrambler_seed) -> np.ndarray:
    """pack_header_fields (modulate/ofdm_frame.rs:668-682): the 14 header bytes, big-endian."""
    if not (0 <= int(mcs_index) <= 255 and 0 <= int(flags) <= 255):
        raise ValueError("mcs_index and flags are bytes")
    f = np.array([_u32(mcs_index, "mcs_index"), _u32(payload_len, "payload_len"), _u32(sequence_num, "sequence_num"),
                  _u32(flags, "flags"), _u32(scrambler_seed, "scrambler_seed")], np.uint32)
    out = np.zeros(HEADER_FIELD_BYTES, np.uint8)
    _arg_check(_L.orion_frame_pack_header(f.ctypes.data, out.ctypes.data))
    return out


def unpack_header_fields(data):
    """The inverse: (mcs_index, payload_len, sequence_num, flags, scrambler_seed)."""
    b = _bytes_arg(data)
    if b.size != HEADER_FIELD_BYTES:
        raise ValueError("a header is 14 field bytes")
    f = np.zeros(5, np.uint32)
    _arg_check(_L.orion_frame_unpack_header(b.ctypes.data, f.ctypes.data))
    return tuple(int(v) for v in f)


def scrambler_seed(width, raw) -> int:
    """build_scrambler's seed (modulate/ofdm_frame.rs:277-289): raw reduced to width bits (all 32
    when width >= 32), a zero mapped to 1."""
    return int(_L.orion_frame_reduce_seed(_u32(width, "width"), _u32(raw, "raw")))


def scramble_bytes(scheme, data, per_frame_seed=0) -> np.ndarray:
    """scramble_bytes (modulate/ofdm_frame.rs:300-312) of the scheme's scrambler: self-inverse."""
    s, b = _frame_scheme(scheme), _bytes_arg(data).copy()
    _arg_check(_L.orion_frame_scramble_bytes(s._ptr(), _u32(per_frame_seed, "per_frame_seed"), b.ctypes.data, b.size))
    return b


def scramble_bits(scheme, bits, per_frame_seed=0) -> np.ndarray:
    """scramble_bits (modulate/ofdm_frame.rs:650-655): an Additive scrambler over bits packed MSB
    first, so bit i meets PN step 8 (i // 8) + 7 - i % 8; other kinds leave the bits alone."""
    s, b = _frame_scheme(scheme), _bytes_arg(bits, "bits").copy()
    _arg_check(_L.orion_frame_scramble_bits(s._ptr(), _u32(per_frame_seed, "per_frame_seed"), b.ctypes.data, b.size))
    return b


def apply_pn_to_llrs(scheme, llr, per_frame_seed=0) -> np.ndarray:
    """apply_pn_to_llrs (demodulate/ofdm_frame.rs:767-779): the sign of llr[i] flipped where
    scramble_bits flips bit i."""
    s = _frame_scheme(scheme)
    l = np.ascontiguousarray(llr, np.float32).copy()
    if l.ndim != 1:
        raise ValueError("llr: expected a 1-D float32 array")
    _arg_check(_L.orion_frame_apply_pn_to_llrs(s._ptr(), _u32(per_frame_seed, "per_frame_seed"), l.ctypes.data, l.size))
    return l


class BlockPlan:
    """BlockPlan (modulate/ofdm_frame.rs:320-334): every intermediate length of one block."""
    __slots__ = ("info_bytes", "framed_bytes", "outer_coded_bits", "outer_il_bits", "inner_coded_bits", "coded_bits")

    def __init__(self, *v):
        for name, x in zip(self.__slots__, v):
            setattr(self, name, int(x))

    def astuple(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, BlockPlan) and self.astuple() == other.astuple()

    def __repr__(self):
        return "BlockPlan(" + ", ".join(f"{n}={getattr(self, n)}" for n in self.__slots__) + ")"


def block_plan(info_bytes, scheme) -> BlockPlan:
    """block_plan (modulate/ofdm_frame.rs:362-427)."""
    info_bytes = int(info_bytes)
    if info_bytes < 0:
        raise ValueError("info_bytes: not negative")
    c = scheme._c if isinstance(scheme, FrameScheme) else None
    if c is None:
        raise ValueError("scheme: a FrameScheme")
    v = (C.c_size_t * 6)()
    _arg_check(_L.orion_frame_block_plan(C.byref(c), info_bytes, v))
    return BlockPlan(*v)


def symbols_for_coded_bits(n_data_carriers, bits_per_carrier, bits) -> int:
    """symbols_for_coded_bits (modulate/ofdm_frame.rs:431-438)."""
    bps = int(n_data_carriers) * int(bits_per_carrier)
    return -(-int(bits) // bps)


def encode_chain_stages(data, scheme, per_frame_seed=0):
    """encode_chain_stages (modulate/ofdm_frame.rs:572-615) on the host: (outer_il_bits, coded)."""
    s, b = _frame_scheme(scheme), _bytes_arg(data)
    p = block_plan(b.size, s)
    coded, oil = np.zeros(p.coded_bits, np.uint8), np.zeros(p.outer_il_bits, np.uint8)
    _arg_check(_L.orion_frame_encode_chain(s._ptr(), b.ctypes.data, b.size, _u32(per_frame_seed, "per_frame_seed"),
                                           coded.ctypes.data, oil.ctypes.data))
    return oil, coded


def encode_chain(data, scheme, per_frame_seed=0) -> np.ndarray:
    """encode_chain (modulate/ofdm_frame.rs:621-646) on the host: the coded bits of one block."""
    return encode_chain_stages(data, scheme, per_frame_seed)[1]


class ChainOutcome:
    """ChainOutcome (demodulate/ofdm_frame.rs:559-644)."""

    def __init__(self, data, inner_ok, outer_ok, crc_ok, crc_present, outer_present, outer_corrected_bytes,
                 inner_out_bits):
        self.bytes, self.inner_ok, self.outer_ok, self.crc_ok = data, bool(inner_ok), bool(outer_ok), bool(crc_ok)
        self.crc_present, self.outer_present = bool(crc_present), bool(outer_present)
        self.outer_corrected_bytes, self.inner_out_bits = outer_corrected_bytes, inner_out_bits

    def is_valid(self) -> bool:
        return self.crc_ok if self.crc_present else self.outer_ok if self.outer_present else self.inner_ok


def decode_chain(llr, info_bytes, scheme, per_frame_seed=0, ldpc_rule="sum_product"):
    """decode_chain (demodulate/ofdm_frame.rs:651-725) on the host under block_plan(info_bytes,
    scheme): float32 LLRs, positive meaning bit 0 -> a ChainOutcome; raises
    RxError("malformed_header") when too few bits come out of the decoders."""
    s = _frame_scheme(scheme)
    r, scale = _ldpcf_rule(ldpc_rule)
    l = np.ascontiguousarray(llr, np.float32)
    if l.ndim != 1:
        raise ValueError("llr: expected a 1-D float32 array")
    p = block_plan(info_bytes, s)
    cap = max(p.coded_bits, p.outer_il_bits, l.size) + 1024
    data, inner = np.zeros(p.info_bytes, np.uint8), np.zeros(cap, np.uint8)
    out, n_inner = np.zeros(8, np.int32), C.c_size_t(0)
    _arg_check(_L.orion_frame_decode_chain(s._ptr(), l.ctypes.data, l.size, p.info_bytes,
                                           _u32(per_frame_seed, "per_frame_seed"), r, scale, data.ctypes.data,
                                           out.ctypes.data, inner.ctypes.data, cap, C.byref(n_inner)))
    if out[0]:
        raise RxError(int(out[0]))
    return ChainOutcome(data, out[1], out[2], out[3], out[4], out[5], None if out[6] < 0 else int(out[6]),
                        inner[:n_inner.value].copy())


def _frame_i64(x, what, ns, cols, like, dev):
    """x as int64 (ns,) / (ns, cols) where like lives (None stays None)."""
    if x is None:
        return None
    shape = (ns,) if cols is None else (ns, cols)
    if dev:
        import torch

        t = x if _is_torch(x) else torch.as_tensor(np.ascontiguousarray(x, np.int64))
        t = t.to(device=like.device, dtype=torch.int64).contiguous()
    else:
        t = np.ascontiguousarray(x, np.int64)
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: expected shape {shape}")
    return t


def _frame_ptr(a, dev):
    return None if a is None else _rs_ptr(a, dev)


def _contig(a, dev):
    return a.contiguous() if dev else np.ascontiguousarray(a)


def frame_pack_batch(payloads, scheme, fields=None, seeds=None, out_bytes=False, stream=None):
    """The head of the encode chain for a batch on the GPU in one launch, one wave per frame:
    uint8 (nframes, info_len) -> uint8 (nframes, framed * 8) bits, MSB first, or with out_bytes
    (nframes, framed) bytes: append_crc, then scramble_bytes when the scheme's scrambler sits
    before the outer code. fields (payloads None): int64 (nframes, 5) mcs_index, payload_len,
    sequence_num, flags, scrambler_seed, packed as pack_header_fields (a host array is range
    checked as there; of a device tensor the kernel takes the low 8 / 32 bits). seeds: int64 (nframes,)
    per-frame seeds (required by a "per_frame" scrambler). A numpy array (-> numpy) or a
    contiguous torch CUDA tensor (-> a torch tensor on its device, queued on torch's current
    stream or on stream)."""
    s = _frame_scheme(scheme)
    if (payloads is None) == (fields is None):
        raise ValueError("frame_pack_batch: payloads or fields")
    if fields is not None:
        dev = _is_torch(fields)
        ns, info_len = int(fields.shape[0]), HEADER_FIELD_BYTES
        if not dev:  # as pack_header_fields refuses them; a device tensor is not read back: the
            # kernel takes the low 8 bits of mcs_index and flags, the low 32 of the others
            fa = np.asarray(fields)
            if fa.ndim != 2 or fa.shape[1] != 5 or (fa < 0).any() or (fa[:, [0, 3]] > 255).any() or (fa > 0xFFFFFFFF).any():
                raise ValueError("fields: (nframes, 5), mcs_index and flags bytes, the others 0 .. 2^32 - 1")
        f = _frame_i64(fields, "fields", ns, 5, fields, dev)
        p, like = None, f
    else:
        p, dev = _fec2_arg(payloads, "payloads", "uint8", (2,))
        ns, info_len = int(p.shape[0]), int(p.shape[1])
        f, like = None, p
    sd = _frame_seeds(s, seeds, ns, like, dev, s._c.scrambler_pos == 0)
    framed = info_len + s.crc_len
    out = _rs_out(like, dev, (ns, framed if out_bytes else framed * 8), "uint8")
    args = (s._ptr(), _frame_ptr(p, dev), _frame_ptr(f, dev), _frame_ptr(sd, dev), ns, info_len, int(bool(out_bytes)),
            _rs_ptr(out, dev))
    if dev:
        _arg_check(_L.orion_frame_pack_batch_device(*args, SyncEngine._stream(like, stream)))
    else:
        _arg_check(_L.orion_frame_pack_batch(*args))
    return out


def _frame_seeds(s, seeds, ns, like, dev, here):
    """The per-frame seeds a call passes down: required where a "per_frame" scrambler acts."""
    if s.per_frame_seed and here and seeds is None:
        raise ValueError("seeds: the scheme's scrambler takes a seed per frame")
    return _frame_i64(seeds, "seeds", ns, None, like, dev) if s.per_frame_seed and here else None


def frame_unpack_batch(x, info_len, scheme, seeds=None, in_bytes=False, unsat=None, status=None, header=False,
                       stream=None):
    """The tail of the decode chain for a batch on the GPU in one launch, one wave per frame: the
    first framed * 8 elements of each row of x, uint8 (nframes, >= framed * 8), are the framed
    bits (in_bytes: the first framed elements its bytes), as the outer decoders write them.
    They are packed, descrambled (a scrambler before the outer code) and their CRC is checked.
    unsat int32 (nframes, n_inner) and status int32 (nframes, n_outer) are the decoders' per-word
    outputs. Returns a dict: payload uint8 (nframes, info_len), inner_ok (all unsat == 0),
    outer_ok (all status >= 0), crc_ok, valid (ChainOutcome.is_valid) as bool (nframes,),
    corrected int32 (nframes,) the sum of the non-negative status entries, and with header
    (info_len 14) fields int64 (nframes, 5). A numpy array (-> numpy) or a contiguous torch CUDA
    tensor (-> torch tensors on its device, queued on torch's current stream or on stream)."""
    s = _frame_scheme(scheme)
    a, dev = _fec2_arg(x, "x", "uint8", (2,))
    ns, stride, info_len = int(a.shape[0]), int(a.shape[1]), int(info_len)
    if info_len < 0 or stride < (info_len + s.crc_len) * (1 if in_bytes else 8):
        raise ValueError("x: a row holds at least the framed block")
    if header and info_len != HEADER_FIELD_BYTES:
        raise ValueError("a header is 14 field bytes")
    n_in = n_out = 0
    if unsat is not None:
        unsat, d2 = _fec2_arg(unsat, "unsat", "int32", (2,))
        n_in = int(unsat.shape[1])
        if d2 != dev or int(unsat.shape[0]) != ns:
            raise ValueError("unsat: (nframes, n_inner) where x lives")
    if status is not None:
        status, d2 = _fec2_arg(status, "status", "int32", (2,))
        n_out = int(status.shape[1])
        if d2 != dev or int(status.shape[0]) != ns:
            raise ValueError("status: (nframes, n_outer) where x lives")
    sd = _frame_seeds(s, seeds, ns, a, dev, s._c.scrambler_pos == 0)
    payload, flags = _rs_out(a, dev, (ns, info_len), "uint8"), _rs_out(a, dev, (ns, 4), "uint8")
    corrected = _rs_out(a, dev, (ns,), "int32")
    fields = _rs_out(a, dev, (ns, 5), "int64") if header else None
    args = (s._ptr(), _rs_ptr(a, dev), stride, int(bool(in_bytes)), _frame_ptr(sd, dev), _frame_ptr(unsat, dev), n_in,
            _frame_ptr(status, dev), n_out, ns, info_len, _rs_ptr(payload, dev), _rs_ptr(flags, dev),
            _rs_ptr(corrected, dev), _frame_ptr(fields, dev))
    if dev:
        _arg_check(_L.orion_frame_unpack_batch_device(*args, SyncEngine._stream(a, stream)))
    else:
        _arg_check(_L.orion_frame_unpack_batch(*args))
    out = {"payload": payload, "inner_ok": flags[:, 0] != 0, "outer_ok": flags[:, 1] != 0, "crc_ok": flags[:, 2] != 0,
           "valid": flags[:, 3] != 0, "corrected": corrected}
    if header:
        out["fields"] = fields
    return out


def frame_coded_bits_batch(bits, scheme, nbits=None, out_len=None, seeds=None, stream=None):
    """The rows ofdm_modulate_batch takes, for a batch on the GPU in one launch: uint8 (nframes,
    >= nbits) -> uint8 (nframes, out_len): the first nbits elements of each row (default: all),
    scramble_bits applied when the scheme's Additive scrambler sits after the inner code, then
    zeros up to out_len (default nbits). A numpy array (-> numpy) or a contiguous torch CUDA
    tensor (-> a torch tensor on its device, queued on torch's current stream or on stream)."""
    s = _frame_scheme(scheme)
    b, dev = _fec2_arg(bits, "bits", "uint8", (2,))
    ns, stride = int(b.shape[0]), int(b.shape[1])
    nbits = stride if nbits is None else int(nbits)
    out_len = nbits if out_len is None else int(out_len)
    if not 0 <= nbits <= min(stride, out_len):
        raise ValueError("nbits: within a row of bits and within out_len")
    sd = _frame_seeds(s, seeds, ns, b, dev, s._c.scrambler_pos == 1)
    out = _rs_out(b, dev, (ns, out_len), "uint8")
    args = (s._ptr(), _rs_ptr(b, dev), stride, nbits, _frame_ptr(sd, dev), ns, out_len, _rs_ptr(out, dev))
    if dev:
        _arg_check(_L.orion_frame_coded_bits_batch_device(*args, SyncEngine._stream(b, stream)))
    else:
        _arg_check(_L.orion_frame_coded_bits_batch(*args))
    return out


def frame_llr_prepare_batch(llr, n, scheme, seeds=None, stream=None):
    """The mirror of frame_coded_bits_batch: float32 (nframes, >= n), as ofdm_demodulate_batch(...,
    llr=True) gives them -> float32 (nframes, n): the first n LLRs of each row, apply_pn_to_llrs
    applied when the scheme's Additive scrambler sits after the inner code (the sign bit alone
    changes: NaN, zeros and infinities keep every other bit). A numpy array (-> numpy) or a
    contiguous torch CUDA tensor (-> a torch tensor on its device, queued on torch's current
    stream or on stream)."""
    s = _frame_scheme(scheme)
    l, dev = _fec2_arg(llr, "llr", "float32", (2,))
    ns, stride, n = int(l.shape[0]), int(l.shape[1]), int(n)
    if not 0 <= n <= stride:
        raise ValueError("n: within a row of llr")
    sd = _frame_seeds(s, seeds, ns, l, dev, s._c.scrambler_pos == 1)
    out = _rs_out(l, dev, (ns, n), "float32")
    args = (s._ptr(), _rs_ptr(l, dev), stride, n, _frame_ptr(sd, dev), ns, _rs_ptr(out, dev))
    if dev:
        _arg_check(_L.orion_frame_llr_prepare_batch_device(*args, SyncEngine._stream(l, stream)))
    else:
        _arg_check(_L.orion_frame_llr_prepare_batch(*args))
    return out


def frame_bytes_to_bits_batch(x, stream=None):
    """uint8 (nframes, nbytes) -> (nframes, nbytes * 8), MSB first, on the GPU in one launch:
    what joins the byte-domain Reed-Solomon encoder to the bit-domain inner encoders. A numpy
    array (-> numpy) or a contiguous torch CUDA tensor (-> torch, on torch's current stream or
    on stream)."""
    a, dev = _fec2_arg(x, "x", "uint8", (2,))
    ns, nb = int(a.shape[0]), int(a.shape[1])
    out = _rs_out(a, dev, (ns, nb * 8), "uint8")
    if dev:
        _arg_check(_L.orion_frame_bytes_to_bits_batch_device(a.data_ptr(), ns, nb, out.data_ptr(),
                                                             SyncEngine._stream(a, stream)))
    else:
        _arg_check(_L.orion_frame_bytes_to_bits_batch(a.ctypes.data, ns, nb, out.ctypes.data))
    return out


def _frame_device_scheme(s):
    """What the batched chain takes of a scheme; the rest runs on the host path (encode_chain /
    decode_chain) alone."""
    c = s._c
    if c.outer_il == 1:
        raise ValueError("the batched chain takes no outer Block interleaver (the host chain does)")
    if c.outer_il == 2 and c.outer != 2:
        raise ValueError("the batched chain takes the Forney outer interleaver over Reed-Solomon words only")
    if c.inner_il == 2 or (c.inner_il == 1 and c.inner == 0):
        raise ValueError("the batched chain takes a Block inner interleaver fused into an inner code, nothing else")
    inner_il = (int(c.inner_il_a), int(c.inner_il_b)) if c.inner_il == 1 else None
    rate = {v: k for k, v in FEC_RATES.items()}.get(int(c.inner_b))
    code = {v: k for k, v in FEC_CODES.items()}.get(int(c.inner_a))
    return c, inner_il, rate, code


def _pad_cols(a, width, dev):
    if int(a.shape[1]) == width:
        return a
    if dev:
        import torch

        return torch.nn.functional.pad(a, (0, width - int(a.shape[1])))
    return np.pad(a, ((0, 0), (0, width - a.shape[1])))


class _TorchOn:
    """torch's own work (pads, slices, allocations) inside a chain call goes where the launches
    go: with a raw stream handle, torch's current stream is that stream for the call."""

    def __init__(self, like, stream):
        self._ctx = None
        if stream is not None and _is_torch(like):
            import torch

            self._ctx = torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=like.device))

    def __enter__(self):
        if self._ctx is not None:
            self._ctx.__enter__()

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)


def frame_encode_chain_batch(payloads, scheme, fields=None, seeds=None, out_len=None, stream=None):
    """encode_chain for a batch of equal-length blocks on the GPU: uint8 (nframes, info_len) (or
    header fields, see frame_pack_batch) -> uint8 (nframes, out_len) coded bits, zero-padded
    from plan.coded_bits to out_len (default: no padding), row k equal to encode_chain of block k
    under seeds[k]. The launches: frame_pack_batch -> bch_encode_batch / rs_encode_batch ->
    forney_interleave_batch -> ldpc_family_encode_batch / conv_encode_batch (a Block inner
    interleaver fused) -> frame_coded_bits_batch. Not taken (ValueError; the host chain takes
    them): an outer Block interleaver, the Forney interleaver without Reed-Solomon, an inner
    interleaver without an inner code."""
    with _TorchOn(payloads if payloads is not None else fields, stream):
        return _frame_encode_chain(payloads, _frame_scheme(scheme), fields, seeds, out_len, stream)


def _frame_encode_chain(payloads, s, fields, seeds, out_len, stream):
    c, inner_il, rate, code = _frame_device_scheme(s)
    dev = _is_torch(payloads if payloads is not None else fields)
    info_len = HEADER_FIELD_BYTES if payloads is None else int(payloads.shape[1])
    plan = block_plan(info_len, s)
    x = frame_pack_batch(payloads, s, fields=fields, seeds=seeds, out_bytes=c.outer == 2 or c.outer_il == 2,
                         stream=stream)
    ns = int(x.shape[0])
    if c.outer == 1:
        x = bch_encode_batch(x, int(c.outer_a), stream=stream)
    elif c.outer == 2:
        n, k = int(c.outer_a), int(c.outer_a) - int(c.outer_b)
        ncw = -(-plan.framed_bytes // k)
        x = rs_encode_batch(_contig(_pad_cols(x, ncw * k, dev).reshape(ns, ncw, k), dev), n, int(c.outer_b),
                            stream=stream)
        if c.outer_il != 2:
            x = frame_bytes_to_bits_batch(x.reshape(ns, ncw * n), stream=stream)
    if c.outer_il == 2:
        x = forney_interleave_batch(x, int(c.outer_il_a), int(c.outer_il_b), bits=True, stream=stream)
    if c.inner == 1:
        x = ldpc_family_encode_batch(x, {v: k for k, v in LDPC_CODES.items()}[int(c.inner_a)], interleaver=inner_il,
                                     stream=stream)
    elif c.inner == 2:
        x = conv_encode_batch(x, rate, code, interleaver=inner_il, stream=stream)
    if int(x.shape[1]) != plan.coded_bits:
        raise OrionError(f"frame chain: {int(x.shape[1])} coded bits where the plan has {plan.coded_bits}")
    return frame_coded_bits_batch(x, s, out_len=plan.coded_bits if out_len is None else out_len, seeds=seeds,
                                  stream=stream)


def frame_decode_chain_batch(llr, info_len, scheme, seeds=None, ldpc_rule="sum_product", header=False, stream=None):
    """decode_chain for a batch of equal-length blocks on the GPU: float32 (nframes, >=
    plan.coded_bits) LLRs, as ofdm_demodulate_batch(..., llr=True) gives them -> the dict of
    frame_unpack_batch plus inner_out_bits uint8 (nframes, ...), the inner decoder's untrimmed
    output; entry k equals decode_chain of row k under seeds[k] in every field. The launches:
    frame_llr_prepare_batch -> ldpc_family_decode_batch (50 iterations) / conv_viterbi_batch ->
    bch_decode_batch / rs_decode_batch (the Forney deinterleaver fused), over
    plan.outer_coded_bits alone -> frame_unpack_batch. The same schemes as
    frame_encode_chain_batch."""
    with _TorchOn(llr, stream):
        return _frame_decode_chain(llr, info_len, _frame_scheme(scheme), seeds, ldpc_rule, header, stream)


def _frame_decode_chain(llr, info_len, s, seeds, ldpc_rule, header, stream):
    c, inner_il, rate, code = _frame_device_scheme(s)
    plan = block_plan(info_len, s)
    l, dev = _fec2_arg(llr, "llr", "float32", (2,))
    if int(l.shape[1]) < plan.coded_bits:
        raise ValueError(f"llr: a row holds at least the plan's {plan.coded_bits} coded bits")
    if int(l.shape[1]) != plan.coded_bits or (c.scrambler == 1 and c.scrambler_pos == 1):
        l = frame_llr_prepare_batch(l, plan.coded_bits, s, seeds=seeds, stream=stream)
    unsat = None
    if c.inner == 1:
        name = {v: k for k, v in LDPC_CODES.items()}[int(c.inner_a)]
        bits, unsat, _ = ldpc_family_decode_batch(l, name, max_iter=50, rule=ldpc_rule, interleaver=inner_il,
                                                  stream=stream)
        nblk, kk = plan.inner_coded_bits // Ldpc(name).n, Ldpc(name).k
        if int(unsat.shape[1]) != nblk:  # interleaver padding of a block or more is not the code's
            bits, unsat = _contig(bits[:, :nblk * kk], dev), _contig(unsat[:, :nblk], dev)
    elif c.inner == 2:
        bits = conv_viterbi_batch(l, plan.outer_il_bits, rate, code, interleaver=inner_il, stream=stream)
    elif dev:
        import torch

        bits = (l <= 0).to(torch.uint8)
    else:
        bits = (l <= 0).astype(np.uint8)
    inner_out = bits
    x, status, in_bytes = bits, None, False
    if c.outer == 2:
        n = int(c.outer_a)
        de = (int(c.outer_il_a), int(c.outer_il_b)) if c.outer_il == 2 else None
        x = _contig(bits[:, :plan.outer_il_bits if de else plan.outer_coded_bits], dev)
        msgs, status = rs_decode_batch(x, n, int(c.outer_b), bits=True, deinterleave=de, stream=stream)
        x, in_bytes = msgs.reshape(int(msgs.shape[0]), -1), True
    elif c.outer == 1:
        x, status = bch_decode_batch(_contig(bits[:, :plan.outer_coded_bits], dev), int(c.outer_a), stream=stream)
    out = frame_unpack_batch(x, info_len, s, seeds=seeds, in_bytes=in_bytes, unsat=unsat, status=status,
                             header=header, stream=stream)
    out["inner_out_bits"] = inner_out
    return out


# ---- the COFDM frame layer at a known start: OfdmFrameMod / OfdmFrameDemod
# (src/modulate/ofdm_frame.rs:125-202, 781-987, src/demodulate/ofdm_frame.rs:862-1255,
# src/sync/ofdm_sync.rs:142-352, src/fec/frame.rs) ----
_L.orion_frame_assemble_batch_device.restype = C.c_int
_L.orion_frame_assemble_batch_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                 C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                 C.c_void_p]
HEADER_CONSTELLATION, HEADER_LDPC = "bpsk", "n512r12"  # modulate/ofdm_frame.rs:131-135
__all__ += ["RxError", "FrameMetadata", "FramePacket", "Mcs", "McsTable", "OfdmPreamble", "generate_ofdm_preamble",
            "OfdmFrameMod", "OfdmFrameDemod", "frame_assemble_batch", "HEADER_CONSTELLATION", "HEADER_LDPC"]


class FrameMetadata:
    """FrameMetadata (fec/frame.rs:41-56)."""

    def __init__(self, sequence_num=0, mcs_index=0, flags=0):
        self.sequence_num, self.mcs_index, self.flags = _u32(sequence_num, "sequence_num"), int(mcs_index), int(flags)
        if not (0 <= self.mcs_index <= 255 and 0 <= self.flags <= 255):
            raise ValueError("mcs_index and flags are bytes")

    def __eq__(self, o):
        return isinstance(o, FrameMetadata) and (self.sequence_num, self.mcs_index, self.flags) == \
            (o.sequence_num, o.mcs_index, o.flags)

    def __repr__(self):
        return f"FrameMetadata(sequence_num={self.sequence_num}, mcs_index={self.mcs_index}, flags={self.flags})"


class FramePacket:
    """FramePacket (fec/frame.rs:24-34): metadata plus the payload bytes."""

    def __init__(self, metadata, payload):
        self.metadata = metadata
        self.payload = _bytes_arg(np.frombuffer(bytes(payload), np.uint8) if isinstance(payload, (bytes, bytearray))
                                  else payload, "payload").copy()

    def __eq__(self, o):
        return isinstance(o, FramePacket) and self.metadata == o.metadata and np.array_equal(self.payload, o.payload)


class Mcs:
    """Mcs (modulate/ofdm_frame.rs:140-159): the payload's constellation, inner and outer FEC,
    the codes in FrameScheme's vocabulary."""

    def __init__(self, constellation, inner=None, outer=None):
        _ofdm_order(constellation)
        FrameScheme(inner=inner, outer=outer)
        self.constellation, self.inner, self.outer = constellation, inner, outer


class McsTable:
    """McsTable (modulate/ofdm_frame.rs:163-202): mcs_index -> Mcs; both ends share it."""

    def __init__(self, entries=()):
        self.entries = list(entries)

    @classmethod
    def default_ladder(cls) -> "McsTable":
        return cls([Mcs(c, ("ldpc", "n512r12"), ("bch", 8)) for c in ("bpsk", "qpsk", "qam16", "qam64")])

    def add(self, constellation, inner=None, outer=None) -> int:
        if len(self.entries) >= 256:
            raise ValueError("an MCS table holds at most 256 entries")
        self.entries.append(Mcs(constellation, inner, outer))
        return len(self.entries) - 1

    def get(self, mcs_index):
        return self.entries[mcs_index] if 0 <= mcs_index < len(self.entries) else None

    def __len__(self):
        return len(self.entries)


class OfdmPreamble:
    """OfdmPreamble (sync/ofdm_sync.rs): num_repeats raw repeats of repeat_len samples, then an
    optional training symbol of training_n_fft + training_cp_len samples."""

    def __init__(self, num_repeats, repeat_len):
        self.num_repeats, self.repeat_len, self.training = int(num_repeats), int(repeat_len), None
        if self.num_repeats < 0 or self.repeat_len < 0:
            raise ValueError("OfdmPreamble: counts are not negative")

    def with_training_symbol(self, n_fft, cp_len) -> "OfdmPreamble":
        p = OfdmPreamble(self.num_repeats, self.repeat_len)
        p.training = (int(n_fft), int(cp_len))
        return p

    @property
    def total_len(self) -> int:
        return self.num_repeats * self.repeat_len + (sum(self.training) if self.training else 0)


def _unit_sequence(n, seed):
    """pseudo_random_unit_sequence (ofdm_sync.rs:335-352): xorshift64, each part +-1/sqrt(2) by the
    sign of (state as f32) / 2^64 - 0.5."""
    state, mask, out = seed, (1 << 64) - 1, np.zeros(n, np.complex64)
    h = np.float32(0.70710678118654752440)  # FRAC_1_SQRT_2

    def nxt():
        nonlocal state
        state ^= (state << 13) & mask
        state ^= state >> 7
        state ^= (state << 17) & mask
        return np.float32(np.float32(np.uint64(state)) / np.float32(2.0 ** 64)) - np.float32(0.5)

    for i in range(n):
        re = h if nxt() >= 0 else -h
        im = h if nxt() >= 0 else -h
        out[i] = complex(re, im)
    return out


def _cf32_scale(x, g):
    g = np.float32(g)
    out = np.empty(x.shape, np.complex64)
    out.real, out.imag = x.real * g, x.imag * g
    return out


def generate_ofdm_preamble(cfg, num_repeats, repeat_len, training_n_fft=None, training_cp_len=None) -> np.ndarray:
    """generate_ofdm_preamble (sync/ofdm_sync.rs:142-332) on the host: the band-limited repeat base
    (bins that are multiples of n_fft / repeat_len inside the occupied span, DC skipped, scaled
    to twice a data symbol's RMS), or the wideband sequence when the geometry admits none;
    then the training symbol loaded on the plan's occupied bins alone; cfg.gain applied."""
    n_fft, half, n_data = cfg.n_fft, cfg.occupied_half_carriers, cfg.num_data_carriers
    repeat_len, num_repeats = int(repeat_len), int(num_repeats)
    base = None
    if repeat_len > 0 and n_fft % repeat_len == 0 and half > 0:
        k = n_fft // repeat_len
        loaded = [b for i in range(1, half + 1) for b in (i, n_fft - i) if i % k == 0]
        if loaded:
            freq = np.zeros(n_fft, np.complex64)
            freq[loaded] = _unit_sequence(len(loaded), 0x4F46444D50524531)
            t = fft_host(freq, n_fft, inverse=True)[:repeat_len]
            acc = np.float32(0.0)
            for c in t:
                acc = np.float32(acc + np.float32(np.float32(c.real * c.real) + np.float32(c.imag * c.imag)))
            rms = np.sqrt(np.float32(acc / np.float32(repeat_len)))
            if rms > 0:
                target = np.float32(np.float32(np.float32(2.0) * np.sqrt(np.float32(n_data))) / np.float32(n_fft))
                t = _cf32_scale(t, np.float32(target / rms))
            base = t
    if base is None:
        base = _unit_sequence(repeat_len, 0x4F46444D50524531)
    parts = [base] * num_repeats
    if training_n_fft is not None:
        tn, tcp = int(training_n_fft), int(training_cp_len or 0)
        freq = ofdm_tables(n_fft=tn)[2]
        occ = cfg.occupied_bins()
        if occ.size:
            load = np.zeros(tn, bool)
            load[occ[occ < tn]] = True
            freq = np.where(load, freq, np.complex64(0)).astype(np.complex64)
        t = fft_host(np.ascontiguousarray(freq), tn, inverse=True)
        parts.append(np.concatenate([t[tn - tcp:], t]) if tcp else t)
    out = np.concatenate(parts).astype(np.complex64) if parts else np.zeros(0, np.complex64)
    return _cf32_scale(out, cfg.gain) if np.float32(cfg.gain) != np.float32(1.0) else out


def frame_assemble_batch(lead, header_iq, payload_iq, sps, win_start, ramp=None, stream=None):
    """The frames' IQ on the GPU in one launch: complex64 lead (lead_len,) shared by all frames,
    header_iq (nframes, hdr_len), payload_iq (nframes, pay_len) -> (nframes, frame_len). With
    ramp (SymbolWindow's, float32) every whole symbol of sps samples from win_start on is
    tapered on its first and last len(ramp) samples, the frame modulator's window post-pass.
    Contiguous torch CUDA tensors, queued on torch's current stream or on stream."""
    import torch

    for t, nd, dt in ((lead, 1, torch.complex64), (header_iq, 2, torch.complex64), (payload_iq, 2, torch.complex64)):
        if not _is_torch(t) or not t.is_cuda or not t.is_contiguous() or t.dim() != nd or t.dtype != dt:
            raise ValueError("frame_assemble_batch: contiguous complex64 CUDA tensors, lead 1-D, the others 2-D")
    ns = int(header_iq.shape[0])
    if int(payload_iq.shape[0]) != ns:
        raise ValueError("frame_assemble_batch: one header and one payload row per frame")
    nr = 0 if ramp is None else int(ramp.numel())
    if nr and (not ramp.is_cuda or not ramp.is_contiguous() or ramp.dtype != torch.float32):
        raise ValueError("ramp: a contiguous float32 CUDA tensor")
    ll, hl, pl = int(lead.numel()), int(header_iq.shape[1]), int(payload_iq.shape[1])
    out = torch.empty((ns, ll + hl + pl), dtype=torch.complex64, device=header_iq.device)
    _arg_check(_L.orion_frame_assemble_batch_device(lead.data_ptr(), ll, header_iq.data_ptr(), hl, payload_iq.data_ptr(),
                                                    pl, ns, int(sps), int(win_start), ramp.data_ptr() if nr else None,
                                                    nr, out.data_ptr(), SyncEngine._stream(header_iq, stream)))
    return out


class _FrameLayer:
    """What the frame modulator and demodulator share: the schemes, plans and symbol-layer
    handles of a configuration and an MCS table."""

    def __init__(self, cfg, mcs_table):
        if not isinstance(cfg, OfdmConfig) or not isinstance(mcs_table, McsTable) or len(mcs_table) < 1:
            raise ValueError("an OfdmConfig and an McsTable of at least one entry")
        if cfg.rf_hz != 0.0:  # assert_baseband, modulate/ofdm_frame.rs:815-822
            raise ValueError(f"OFDM frame assembly is baseband-only: got rf_hz = {cfg.rf_hz} Hz. Modulate at rf_hz = 0.0 "
                             "and upconvert the whole burst with one continuous Rotator.")
        cfg.validate_frame()
        self.cfg, self.mcs_table, self.f = cfg, mcs_table, cfg.frame_fields
        self.sps, self.n_data = cfg.samples_per_ofdm_symbol, cfg.num_data_carriers
        self.header_scheme = FrameScheme(crc=self.f["header_crc"], inner=("ldpc", HEADER_LDPC))
        self.header_plan = block_plan(HEADER_FIELD_BYTES, self.header_scheme)
        self.header_symbols = symbols_for_coded_bits(self.n_data, 1, self.header_plan.coded_bits)
        self._sym, self._mods, self._demods = {}, {}, {}

    def scheme(self, mcs) -> FrameScheme:
        f = self.f
        return FrameScheme(crc=f["payload_crc"], outer=mcs.outer, inner=mcs.inner, outer_interleaver=f["outer_interleaver"],
                           inner_interleaver=f["inner_interleaver"], scrambler=f["scrambler"],
                           scrambler_pos=f["scrambler_pos"])

    def payload_symbols(self, mcs, plan) -> int:
        return symbols_for_coded_bits(self.n_data, (1, 2, 4, 6, 8)[_ofdm_order(mcs.constellation)], plan.coded_bits)

    def symcfg(self, constellation):
        if constellation not in self._sym:
            self._sym[constellation] = self.cfg.symbol_config(constellation)
        return self._sym[constellation]

    def mod(self, constellation):
        if constellation not in self._mods:
            self._mods[constellation] = OfdmMod(self.symcfg(constellation))
        return self._mods[constellation]

    def demod(self, constellation):
        if constellation not in self._demods:
            self._demods[constellation] = OfdmDemod(self.symcfg(constellation), equalizer=None)
        return self._demods[constellation]

    def _device_ok(self):
        if self.f["tx_lowpass"] is not None:
            raise ValueError("the batched path takes no TX low-pass (the host path does)")


class OfdmFrameMod(_FrameLayer):
    """OfdmFrameMod (modulate/ofdm_frame.rs:781-987): FramePacket -> IQ,
    [S&C repeats + training symbol][header: BPSK, n512r12, header_crc][payload per its MCS],
    every CP-bearing symbol from the training symbol on tapered once when the plan has a window
    roll-off, then the TX low-pass when one is set. modulate_frame is the library's host code;
    modulate_frames the same frames batched on the GPU."""

    def __init__(self, cfg, mcs_table, preamble):
        super().__init__(cfg, mcs_table)
        if not isinstance(preamble, OfdmPreamble):
            raise ValueError("preamble: an OfdmPreamble")
        self.preamble = preamble
        tr = preamble.training or (None, None)
        self._lead = generate_ofdm_preamble(cfg, preamble.num_repeats, preamble.repeat_len, tr[0], tr[1])
        self._win_start = preamble.num_repeats * preamble.repeat_len
        self._roll = cfg.window_roll_off
        self._dev = {}

    def frame_len(self, mcs_index, payload_len) -> int:
        mcs = self.mcs_table.get(mcs_index)
        if mcs is None:
            raise ValueError("mcs_index must be in the MCS table")
        return self._lead.size + (self.header_symbols + self.payload_symbols(mcs, block_plan(payload_len, self.scheme(mcs)))) * self.sps

    def _window(self, out):
        if self._roll == 0 or out.size <= self._win_start:
            return out
        k = (out.size - self._win_start) // self.sps
        end = self._win_start + k * self.sps
        out[self._win_start:end] = ofdm_window(np.ascontiguousarray(out[self._win_start:end]), self.sps, self._roll)
        return out

    def modulate_frame(self, frame, per_frame_seed=0) -> np.ndarray:
        """modulate_frame (modulate/ofdm_frame.rs:867-958) on the host."""
        md = frame.metadata
        mcs = self.mcs_table.get(md.mcs_index)
        if mcs is None:
            raise ValueError("mcs_index must be in the MCS table")
        seed = _u32(per_frame_seed, "per_frame_seed")
        fields = pack_header_fields(md.mcs_index, frame.payload.size, md.sequence_num, md.flags, seed)
        hdr = self.mod(HEADER_CONSTELLATION).modulate_host(encode_chain(fields, self.header_scheme, 0))
        pay = self.mod(mcs.constellation).modulate_host(encode_chain(frame.payload, self.scheme(mcs), seed))
        out = self._window(np.concatenate([self._lead, hdr, pay]).astype(np.complex64))
        lp = self.f["tx_lowpass"]
        return lp.apply(out) if lp is not None else out

    def modulate_frames(self, payloads, mcs_index, sequence_nums=None, flags=None, seeds=None, stream=None):
        """A batch sharing one MCS and one payload length on the GPU: uint8 (nframes,
        payload_len) -> complex64 (nframes, frame_len), row k equal to modulate_frame of frame k
        (sequence_nums[k], flags[k], seeds[k]; default 0). The launches: the header and payload
        chains (frame_encode_chain_batch), ofdm_modulate_batch for each, frame_assemble_batch.
        numpy in -> numpy out; a contiguous torch CUDA tensor stays resident, queued on torch's
        current stream or on stream."""
        import torch

        self._device_ok()
        mcs = self.mcs_table.get(int(mcs_index))
        if mcs is None:
            raise ValueError("mcs_index must be in the MCS table")
        if not _is_torch(payloads):
            p, _ = _fec2_arg(payloads, "payloads", "uint8", (2,))
            return self.modulate_frames(torch.from_numpy(p).cuda(), mcs_index, sequence_nums, flags, seeds, stream).cpu().numpy()
        p, _ = _fec2_arg(payloads, "payloads", "uint8", (2,))
        with _TorchOn(p, stream):
            ns, n = int(p.shape[0]), int(p.shape[1])
            sch = self.scheme(mcs)
            plan = block_plan(n, sch)

            def col(x, what):
                if x is None:
                    return torch.zeros(ns, dtype=torch.int64, device=p.device)
                return _frame_i64(x, what, ns, None, p, True)

            sd = col(seeds, "seeds")
            fields = torch.stack([torch.full((ns,), int(mcs_index), dtype=torch.int64, device=p.device),
                                  torch.full((ns,), n, dtype=torch.int64, device=p.device),
                                  col(sequence_nums, "sequence_nums"), col(flags, "flags"), sd], dim=1).contiguous()
            hmod, pmod = self.mod(HEADER_CONSTELLATION), self.mod(mcs.constellation)
            hbits = frame_encode_chain_batch(None, self.header_scheme, fields=fields,
                                             out_len=self.header_symbols * hmod.bits_per_ofdm_symbol, stream=stream)
            pbits = frame_encode_chain_batch(p, sch, seeds=sd if sch.per_frame_seed else None,
                                             out_len=self.payload_symbols(mcs, plan) * pmod.bits_per_ofdm_symbol,
                                             stream=stream)
            hiq = ofdm_modulate_batch(hmod, hbits, stream=stream)
            piq = ofdm_modulate_batch(pmod, pbits, stream=stream)
            key = str(p.device)
            if key not in self._dev:  # the shared lead and the ramp, uploaded once per modulator
                ramp = ofdm_tables(symbol_len=self.sps, roll_off=self._roll)[4]
                self._dev[key] = (torch.from_numpy(self._lead).to(p.device), torch.from_numpy(ramp).to(p.device))
            lead, ramp = self._dev[key]
            return frame_assemble_batch(lead, hiq, piq, self.sps, self._win_start, ramp if ramp.numel() else None,
                                        stream=stream)


class OfdmFrameDemod(_FrameLayer):
    """OfdmFrameDemod at a known start (demodulate/ofdm_frame.rs:862-1255 with no channel
    estimate): IQ from the first sample after the preamble and training symbol -> FramePacket.
    decode is the library's host code and raises RxError; decode_frames decodes a batch on the
    GPU and reports the same outcome per frame."""

    def _llrs_host(self, constellation, iq, n_sym):
        soft = self.demod(constellation).process_host(np.ascontiguousarray(iq[:n_sym * self.sps]))
        return ofdm_llr(constellation, soft)

    def decode(self, iq) -> FramePacket:
        """decode (demodulate/ofdm_frame.rs:1231-1254): truncated input -> malformed_header, an
        invalid header -> header_crc_mismatch, an MCS index outside the table ->
        malformed_header, an invalid payload -> crc_mismatch; the payload is trimmed to the
        declared length. The header is decoded under sum-product whatever the payload's rule."""
        iq = _ofdm_arr(iq, np.complex64, "iq")
        nh = self.header_symbols
        if iq.size < nh * self.sps:
            raise RxError("malformed_header")
        header = decode_chain(self._llrs_host(HEADER_CONSTELLATION, iq, nh), HEADER_FIELD_BYTES, self.header_scheme, 0,
                              "sum_product")
        if not header.is_valid():
            raise RxError("header_crc_mismatch")
        mcs_index, payload_len, seq, flags, seed = unpack_header_fields(header.bytes)
        mcs = self.mcs_table.get(mcs_index)
        if mcs is None:
            raise RxError("malformed_header")
        sch = self.scheme(mcs)
        try:
            plan = block_plan(payload_len, sch)
        except ValueError:
            raise RxError("malformed_header") from None
        n_sym = self.payload_symbols(mcs, plan)
        body = iq[nh * self.sps:]
        if body.size < n_sym * self.sps:
            raise RxError("malformed_header")
        out = decode_chain(self._llrs_host(mcs.constellation, body, n_sym), payload_len, sch, seed,
                           self.f["ldpc_decode_rule"])
        if not out.is_valid():
            raise RxError("crc_mismatch")
        return FramePacket(FrameMetadata(seq, mcs_index, flags), out.bytes[:payload_len])

    def decode_frames(self, iq, stream=None) -> dict:
        """A batch on the GPU: complex64 (nframes, n), each row from the first sample after the
        preamble and training symbol. Every header is decoded on the device; the parsed fields
        and their validity come to the host in one small copy (the one synchronisation: the
        payload geometry is data); frames are grouped by (mcs_index, payload_len) and each
        group's payload chain is launched. Returns numpy arrays per frame: error (0 or the
        RX_ERRORS code decode raises), mcs_index, sequence_num, flags, payload_len, inner_ok,
        outer_ok, crc_ok, and payloads, a list of uint8 arrays (empty where error != 0). numpy
        or a contiguous torch CUDA tensor, queued on torch's current stream or on stream."""
        import torch

        if not _is_torch(iq):
            if not isinstance(iq, np.ndarray) or iq.dtype != np.complex64 or iq.ndim != 2:
                raise ValueError("iq: expected a 2-D complex64 array")
            return self.decode_frames(torch.from_numpy(np.ascontiguousarray(iq)).cuda(), stream)
        if not iq.is_cuda or not iq.is_contiguous() or iq.dtype != torch.complex64 or iq.dim() != 2:
            raise ValueError("iq: expected a contiguous 2-D complex64 CUDA tensor")
        def llr_of(constellation, block, idx):
            return ofdm_demodulate_batch(self.demod(constellation), block, bits=False, llr=True, stream=stream)[2]

        res, incomplete = self._decode_rows(iq, stream, llr_of)
        res["error"][incomplete] = RX_ERRORS["malformed_header"]  # truncated input, as decode reports it
        return res

    def _decode_rows(self, iq, stream, llr_of, avail=None):
        """What decode_frames and OfdmBurstDemod.receive_frames share: rows (nframes, n) on the
        device, each from the first sample after the preamble and training symbol. The headers
        are decoded on the device, the parsed fields come to the host in one small copy, the
        frames are grouped by (mcs_index, payload_len) and each group's payload chain is launched.
        llr_of(constellation, block, idx) gives the LLRs of block (k, whole symbols), rows idx of
        iq (None: every row). avail (int tensor, nframes): the samples a row really holds (default
        n). Returns (the result dict, incomplete): incomplete marks rows with too few samples for
        the header or for the payload their header declares; nothing else is set for them."""
        import torch

        ns, n = int(iq.shape[0]), int(iq.shape[1])
        res = {k: np.zeros(ns, np.int64) for k in ("error", "mcs_index", "sequence_num", "flags", "payload_len")}
        res.update({k: np.zeros(ns, bool) for k in ("inner_ok", "outer_ok", "crc_ok")})
        res["payloads"] = [np.zeros(0, np.uint8) for _ in range(ns)]
        incomplete = np.zeros(ns, bool)
        hl = self.header_symbols * self.sps
        if n < hl or ns == 0:
            incomplete[:] = True
            return res, incomplete
        with _TorchOn(iq, stream):
            hllr = llr_of(HEADER_CONSTELLATION, iq[:, :hl].contiguous(), None)
            h = frame_decode_chain_batch(hllr, HEADER_FIELD_BYTES, self.header_scheme, ldpc_rule="sum_product",
                                         header=True, stream=stream)
            if stream is not None:
                torch.cuda.current_stream(iq.device).synchronize()
            cols = [h["fields"], h["valid"].to(torch.int64)[:, None]]
            if avail is not None:
                cols.append(avail.to(torch.int64)[:, None])
            head = torch.cat(cols, dim=1).cpu().numpy()  # the one copy
            have = head[:, 6] if avail is not None else np.full(ns, n, np.int64)
            E = RX_ERRORS
            incomplete |= have < hl
            valid = (head[:, 5] != 0) & ~incomplete
            res["error"][~valid & ~incomplete] = E["header_crc_mismatch"]
            for col, key in ((0, "mcs_index"), (1, "payload_len"), (2, "sequence_num"), (3, "flags")):
                res[key][valid] = head[valid, col]
            known = valid & (head[:, 0] < len(self.mcs_table)) & (head[:, 1] <= (1 << 16))  # the device chain's block limit
            res["error"][valid & ~known] = E["malformed_header"]
            key = head[:, 0] * (1 << 33) + head[:, 1]
            groups = {(int(v) >> 33, int(v) & ((1 << 33) - 1)): np.flatnonzero(known & (key == v)) for v in np.unique(key[known])}
            for (mcs_index, plen), rows in groups.items():
                mcs = self.mcs_table.get(mcs_index)
                sch = self.scheme(mcs)
                plen_sym = self.payload_symbols(mcs, block_plan(plen, sch)) * self.sps
                short = (have[rows] - hl < plen_sym) | (n - hl < plen_sym)
                incomplete[rows[short]] = True
                rows = rows[~short]
                if rows.size == 0:
                    continue
                idx = torch.from_numpy(rows).to(iq.device)
                body = iq.index_select(0, idx)[:, hl:hl + plen_sym].contiguous()
                llr = llr_of(mcs.constellation, body, idx)
                seeds = h["fields"].index_select(0, idx)[:, 4].contiguous() if sch.per_frame_seed else None
                out = frame_decode_chain_batch(llr, plen, sch, seeds=seeds, ldpc_rule=self.f["ldpc_decode_rule"], stream=stream)
                if stream is not None:
                    torch.cuda.current_stream(iq.device).synchronize()
                pay = out["payload"].cpu().numpy()
                flg = torch.stack([out["inner_ok"], out["outer_ok"], out["crc_ok"], out["valid"]], dim=1).cpu().numpy()
                res["inner_ok"][rows], res["outer_ok"][rows], res["crc_ok"][rows] = flg[:, 0], flg[:, 1], flg[:, 2]
                res["error"][rows[~flg[:, 3]]] = E["crc_mismatch"]
                for j in np.flatnonzero(flg[:, 3]):
                    res["payloads"][rows[j]] = pay[j]
        return res, incomplete


# ---- OFDM burst acquisition: the Schmidl & Cox packet search, fractional and integer carrier
# offset (src/sync/ofdm_sync.rs:354-589) ----
class _PreambleC(C.Structure):
    _fields_ = [("num_repeats", C.c_size_t), ("repeat_len", C.c_size_t), ("training", C.c_int32),
                ("training_n_fft", C.c_size_t), ("training_cp_len", C.c_size_t)]


class _SyncOutC(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("p", "r", "score", "cfo_hz", "r_peak", "top_start", "top_bins", "accepted_start",
                                          "accepted_in_top", "accepted_bins", "accepted_score", "accepted_cfo_hz")]


_SYNC_RESULT = np.dtype([("start_sample", np.int64), ("cfo_hz", np.float32), ("integer_cfo_bins", np.int32),
                         ("score", np.float32), ("reserved", np.uint32)])
OFDM_SYNC_TOP = 5


def _acquire_sigs():
    vp, sz, f, i, pp = C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.POINTER(_PreambleC)
    sig = {
        "orion_ofdm_sync_offsets": (sz, [sz, f, pp, sz, sz]),
        "orion_ofdm_sync_host": (i, [vp, sz, f, pp, sz, sz, vp, sz, C.POINTER(sz), C.POINTER(f)]),
        "orion_ofdm_sc_metric_host": (i, [vp, sz, f, pp, sz, sz, vp, vp]),
        "orion_ofdm_earliest_accepted": (i, [vp, sz, f, sz, C.POINTER(C.c_int64)]),
        "orion_ofdm_integer_cfo_host": (i, [vp, sz, f, sz, sz, sz, f, C.POINTER(C.c_int32), vp]),
        "orion_ofdm_acquire_new": (vp, [pp]), "orion_ofdm_acquire_free": (None, [vp]),
        "orion_ofdm_sync_batch_device": (i, [vp, vp, sz, sz, f, sz, sz, f, C.POINTER(_SyncOutC), vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(_L, name)
        fn.restype = res
        fn.argtypes = args


_acquire_sigs()
__all__ += ["OfdmSyncResult", "OFDM_SYNC_TOP", "ofdm_sync", "ofdm_sc_metric", "earliest_accepted", "ofdm_integer_cfo",
            "ofdm_sync_batch"]


class OfdmSyncResult:
    """OfdmSyncResult (sync/ofdm_sync.rs:94-107): the preamble's start, the fractional carrier
    offset in Hz (float32), the integer one in subcarrier spacings and the raw timing score."""

    def __init__(self, start_sample, cfo_hz, integer_cfo_bins, score):
        self.start_sample, self.cfo_hz = int(start_sample), np.float32(cfo_hz)
        self.integer_cfo_bins, self.score = int(integer_cfo_bins), np.float32(score)

    def __repr__(self):
        return (f"OfdmSyncResult(start_sample={self.start_sample}, cfo_hz={self.cfo_hz}, "
                f"integer_cfo_bins={self.integer_cfo_bins}, score={self.score})")


def _preamble_c(preamble) -> _PreambleC:
    if not isinstance(preamble, OfdmPreamble):
        raise ValueError("preamble: an OfdmPreamble")
    tr = preamble.training
    return _PreambleC(preamble.num_repeats, preamble.repeat_len, 1 if tr else 0, tr[0] if tr else 0, tr[1] if tr else 0)


def _search_range(search_start, search_end):
    a, b = int(search_start), int(search_end)
    if a < 0 or b < 0:
        raise ValueError("a search range is not negative")
    return a, min(b, (1 << 63) - 1)


def ofdm_sync(iq, fs, preamble, search_start, search_end) -> list:
    """ofdm_sync (sync/ofdm_sync.rs:361-463) on the host: every offset of iq[search_start:
    min(search_end, len - preamble.total_len)] whose window holds energy, ranked by score (r /
    r_peak) (stable, descending) with the raw score reported; the integer search runs for the
    first five when the preamble has a training symbol. Empty for repeat_len == 0, num_repeats
    < 2, fs <= 0 or a range that holds no offset."""
    iq = _ofdm_arr(iq, np.complex64, "iq")
    pc = _preamble_c(preamble)
    a, b = _search_range(search_start, search_end)
    cap = int(_L.orion_ofdm_sync_offsets(iq.size, float(fs), C.byref(pc), a, b))
    res, count = np.zeros(max(cap, 1), _SYNC_RESULT), C.c_size_t(0)
    _arg_check(_L.orion_ofdm_sync_host(iq.ctypes.data, iq.size, float(fs), C.byref(pc), a, b, res.ctypes.data, cap,
                                       C.byref(count), None))
    return [OfdmSyncResult(r["start_sample"], r["cfo_hz"], r["integer_cfo_bins"], r["score"]) for r in res[:count.value]]


def ofdm_sc_metric(iq, fs, preamble, search_start, search_end):
    """(p complex64, r float32) per offset of ofdm_sync's range, the sums it ranks: P(d) summed
    over the adjacent segment pairs and the energy R(d) of the later segments; host only."""
    iq = _ofdm_arr(iq, np.complex64, "iq")
    pc = _preamble_c(preamble)
    a, b = _search_range(search_start, search_end)
    nd = int(_L.orion_ofdm_sync_offsets(iq.size, float(fs), C.byref(pc), a, b))
    p, r = np.zeros(nd, np.complex64), np.zeros(nd, np.float32)
    if nd:
        _arg_check(_L.orion_ofdm_sc_metric_host(iq.ctypes.data, iq.size, float(fs), C.byref(pc), a, b, p.ctypes.data,
                                                r.ctypes.data))
    return p, r


def earliest_accepted(results, score_threshold, cluster_len):
    """earliest_accepted (sync/ofdm_sync.rs:488-503): of ofdm_sync's ranked results with score >=
    score_threshold, the best-ranked one within cluster_len of the earliest; None without one."""
    results = list(results)
    arr = np.zeros(max(len(results), 1), _SYNC_RESULT)
    for k, r in enumerate(results):
        arr[k] = (r.start_sample, r.cfo_hz, r.integer_cfo_bins, r.score, 0)
    idx = C.c_int64(-1)
    _arg_check(_L.orion_ofdm_earliest_accepted(arr.ctypes.data, len(results), float(score_threshold), int(cluster_len),
                                               C.byref(idx)))
    return results[idx.value] if idx.value >= 0 else None


def ofdm_integer_cfo(iq, fs, n_fft, cp_len, training_start, fractional_cfo_hz, corr=False):
    """estimate_integer_cfo_bins (sync/ofdm_sync.rs:513-562) on the host: the training symbol at
    training_start rotated by -fractional_cfo_hz, transformed at the CP boundary and correlated
    with the known pattern over the shifts -n_fft/2 .. n_fft/2; the lowest shift wins a tie.
    With corr, also |corr|^2 per shift (float32, n_fft + 1)."""
    iq = _ofdm_arr(iq, np.complex64, "iq")
    bins, c2 = C.c_int32(0), np.zeros(int(n_fft) + 1, np.float32)
    _arg_check(_L.orion_ofdm_integer_cfo_host(iq.ctypes.data, iq.size, float(fs), int(n_fft), int(cp_len),
                                              int(training_start), float(fractional_cfo_hz), C.byref(bins), c2.ctypes.data))
    return (int(bins.value), c2) if corr else int(bins.value)


_SYNC_BATCH_KEYS = (("p", "complex64", None), ("r", "float32", None), ("score", "float32", None), ("cfo_hz", "float32", None),
                    ("r_peak", "float32", 1), ("top_start", "int32", OFDM_SYNC_TOP), ("top_bins", "int32", OFDM_SYNC_TOP),
                    ("accepted_start", "int32", 1), ("accepted_in_top", "int32", 1), ("accepted_bins", "int32", 1),
                    ("accepted_score", "float32", 1), ("accepted_cfo_hz", "float32", 1))
_acquire_handles = {}


def _acquire_handle(pc):
    key = (pc.num_repeats, pc.repeat_len, pc.training, pc.training_n_fft, pc.training_cp_len)
    if key not in _acquire_handles:
        h = _L.orion_ofdm_acquire_new(C.byref(pc))
        if not h:
            raise ValueError(_err())
        _acquire_handles[key] = h
    return _acquire_handles[key]


def ofdm_sync_batch(iq, fs, preamble, search_start, search_end, score_threshold=0.5, stream=None) -> dict:
    """ofdm_sync and earliest_accepted for every row of iq (ncap, n) on the GPU, one independent
    search per capture. Returns, per offset of the range (nd = min(search_end, n - total_len) -
    search_start): p complex64, r, score (-1 at an offset ofdm_sync skips) and cfo_hz float32,
    each (ncap, nd); per capture: r_peak, top_start and top_bins (ncap, 5) int32 (the first five
    of ofdm_sync's ranking with their integer offsets; -1 / 0 padded), accepted_start (what
    earliest_accepted(ofdm_sync(..), score_threshold, preamble.total_len) picks; -1: none),
    accepted_in_top (which of the five it is, or -1), accepted_integer_cfo_bins (its top-five
    entry, or 0, as the reference searches the first five only), accepted_score and
    accepted_cfo_hz. p, r, score and the choices carry the host's bits; cfo_hz is the device's
    atan2 (a few ulp from the host's). numpy in -> numpy out; a contiguous 2-D complex64 CUDA
    tensor stays resident, queued on torch's current stream or on stream. The input must be
    finite: NaN and infinities are ordered as the reference orders them on the host only."""
    import torch

    if not _is_torch(iq):
        if not isinstance(iq, np.ndarray) or iq.dtype != np.complex64 or iq.ndim != 2:
            raise ValueError("iq: expected a 2-D complex64 array")
        out = ofdm_sync_batch(torch.from_numpy(np.ascontiguousarray(iq)).cuda(), fs, preamble, search_start, search_end,
                              score_threshold, stream)
        if stream is not None:
            torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}
    if not iq.is_cuda or not iq.is_contiguous() or iq.dtype != torch.complex64 or iq.dim() != 2:
        raise ValueError("iq: expected a contiguous 2-D complex64 CUDA tensor")
    pc = _preamble_c(preamble)
    a, b = _search_range(search_start, search_end)
    ncap, n = int(iq.shape[0]), int(iq.shape[1])
    nd = int(_L.orion_ofdm_sync_offsets(n, float(fs), C.byref(pc), a, b))
    with _TorchOn(iq, stream):
        out, fill = {}, {"top_start": -1, "accepted_start": -1, "accepted_in_top": -1}
        for k, dt, w in _SYNC_BATCH_KEYS:
            shape = (ncap, nd) if w is None else (ncap,) if w == 1 else (ncap, w)
            out[k] = torch.full(shape, fill.get(k, 0), dtype=getattr(torch, dt), device=iq.device)
        if nd and ncap:
            oc = _SyncOutC(*[out[k].data_ptr() for k, _, _ in _SYNC_BATCH_KEYS])
            _arg_check(_L.orion_ofdm_sync_batch_device(_acquire_handle(pc), iq.data_ptr(), ncap, n, float(fs), a, b,
                                                       float(score_threshold), C.byref(oc), SyncEngine._stream(iq, stream)))
    out["accepted_integer_cfo_bins"] = out.pop("accepted_bins")
    return out


# ---- the OFDM burst receiver: acquisition, carrier correction, training equalizer, phase tracker
# (src/demodulate/ofdm_frame.rs:55-274, :862-1090, :1280-1592) ----
for _name, _args in (("orion_ofdm_rotate_block_host", [C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
                     ("orion_ofdm_cpe_host", [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t]),
                     ("orion_ofdm_soft_demap_equalized_host", [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                                               C.c_void_p, C.c_void_p]),
                     ("orion_ofdm_acquire_correct_device", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float,
                                                            C.c_size_t, C.POINTER(_SyncOutC), C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.c_void_p]),
                     ("orion_ofdm_acquire_weights_device", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                                            C.c_void_p, C.c_void_p]),
                     ("orion_ofdm_equalize_track_device", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                                           C.c_void_p, C.c_void_p, C.c_void_p])):
    getattr(_L, _name).restype = C.c_int
    getattr(_L, _name).argtypes = _args
__all__ += ["ofdm_rotate_block", "ofdm_remove_common_phase_error", "BurstStep", "OfdmBurstDemod", "OfdmFrameStreamDemod"]


def ofdm_rotate_block(iq, freq_hz, fs) -> np.ndarray:
    """Rotator(freq_hz, fs).rotate_block(iq) from a fresh oscillator (dsp/rotator.rs:74-84), host only."""
    iq = _ofdm_arr(iq, np.complex64, "iq")
    out = np.zeros(iq.size, np.complex64)
    _check(_L.orion_ofdm_rotate_block_host(float(freq_hz), float(fs), iq.ctypes.data, iq.size, out.ctypes.data))
    return out


def ofdm_remove_common_phase_error(constellation, syms) -> np.ndarray:
    """remove_common_phase_error (demodulate/ofdm_frame.rs:200-274) over complex64 (n_sym, n_data)
    equalized symbols, host only: unchanged below 4 symbols; else the decision-directed loop and
    the least-squares phase ramp taken out per symbol."""
    if not isinstance(syms, np.ndarray) or syms.dtype != np.complex64 or syms.ndim != 2:
        raise ValueError("syms: expected a 2-D complex64 array")
    out = np.ascontiguousarray(syms).copy()
    _arg_check(_L.orion_ofdm_cpe_host(_ofdm_order(constellation), out.ctypes.data, out.shape[0], out.shape[1]))
    return out


class BurstStep:
    """One decoded step of the burst receiver (FrameStep::Decoded with the frame's diagnostics):
    packet (a FramePacket) or error (an RxError), consume_to (samples of the buffer this step
    is done with), cfo_hz (the total carrier offset corrected, float32), timing_offset_samples,
    sync_score, and, for a packet, inner_ok / outer_ok / crc_ok. symbols: the payload's equalized
    symbols after the phase tracker (None on the path without a training symbol)."""

    def __init__(self, packet, error, consume_to, cfo_hz, timing_offset_samples, sync_score, inner_ok=None, outer_ok=None,
                 crc_ok=None, symbols=None):
        self.packet, self.error, self.consume_to = packet, error, int(consume_to)
        self.cfo_hz, self.timing_offset_samples, self.sync_score = np.float32(cfo_hz), int(timing_offset_samples), np.float32(sync_score)
        self.inner_ok, self.outer_ok, self.crc_ok, self.symbols = inner_ok, outer_ok, crc_ok, symbols


class OfdmBurstDemod(OfdmFrameDemod):
    """The burst receiver at an unknown start (try_one_frame, demodulate/ofdm_frame.rs:1463-1592):
    ofdm_sync over the whole buffer, earliest_accepted at score_threshold, the carrier offset
    cfo_hz + bins fs / n_fft taken out by a Rotator from the preamble's start, the channel from
    the training symbol at the data window, then the frame body through the held equalizer and
    the phase tracker (decode_frame_body with a channel estimate). Without a training symbol the
    body takes the known-start path. receive is the library's host code."""

    def __init__(self, cfg, mcs_table, preamble, score_threshold=0.5):
        super().__init__(cfg, mcs_table)
        if not isinstance(preamble, OfdmPreamble):
            raise ValueError("preamble: an OfdmPreamble")
        if preamble.training is not None and preamble.training != (cfg.n_fft, cfg.cp_len):
            raise ValueError("the training symbol must have the plan's n_fft and cp_len")
        self.preamble, self.score_threshold = preamble, float(score_threshold)
        self.n_fft, self.cp_len, self.fs = cfg.n_fft, cfg.cp_len, cfg.fs

    def _window_start(self):
        return self.cp_len - min(self.cfg.rx_window_backoff, self.cp_len)

    def _channel_host(self, corrected):
        """estimate_channel (:1576-1592): the training symbol's transform at the data window."""
        if self.preamble.training is None:
            return None
        t0 = self.preamble.num_repeats * self.preamble.repeat_len
        if corrected.size < t0 + self.n_fft + self.cp_len:
            return None
        w0 = t0 + self._window_start()
        return fft_host(np.ascontiguousarray(corrected[w0:w0 + self.n_fft]), self.n_fft)

    def _demap_host(self, constellation, iq, n_sym, est):
        """soft_demap: (llrs, symbols) or None for too few samples."""
        if iq.size < n_sym * self.sps:
            return None
        if est is None:
            return self._llrs_host(constellation, iq, n_sym), None
        order = _ofdm_order(constellation)
        syms = np.zeros(n_sym * self.n_data, np.complex64)
        llr = np.zeros(syms.size * (1, 2, 4, 6, 8)[order], np.float32)
        x = np.ascontiguousarray(iq[:n_sym * self.sps])
        _arg_check(_L.orion_ofdm_soft_demap_equalized_host(self.cfg._h, order, x.ctypes.data, n_sym, est.ctypes.data,
                                                           syms.ctypes.data, llr.ctypes.data))
        return llr, syms.reshape(n_sym, self.n_data)

    def _body_host(self, body, est):
        """decode_frame_body (:862-1090): None (incomplete), an RxError, or (packet, consumed,
        outcome, symbols)."""
        nh = self.header_symbols
        got = self._demap_host(HEADER_CONSTELLATION, body, nh, est)
        if got is None:
            return None
        try:
            header = decode_chain(got[0], HEADER_FIELD_BYTES, self.header_scheme, 0, "sum_product")
        except RxError as e:
            return e
        if not header.is_valid():
            return RxError("header_crc_mismatch")
        mcs_index, payload_len, seq, flags, seed = unpack_header_fields(header.bytes)
        mcs = self.mcs_table.get(mcs_index)
        if mcs is None:
            return RxError("malformed_header")
        sch = self.scheme(mcs)
        try:
            plan = block_plan(payload_len, sch)
        except ValueError:
            return RxError("malformed_header")
        n_sym = self.payload_symbols(mcs, plan)
        got = self._demap_host(mcs.constellation, body[nh * self.sps:], n_sym, est)
        if got is None:
            return None
        try:
            out = decode_chain(got[0], payload_len, sch, seed, self.f["ldpc_decode_rule"])
        except RxError as e:
            return e
        if not out.is_valid():
            return RxError("crc_mismatch")
        return FramePacket(FrameMetadata(seq, mcs_index, flags), out.bytes[:payload_len]), (nh + n_sym) * self.sps, out, got[1]

    def receive(self, iq):
        """try_one_frame on complex64 iq: None for "need more" (fewer than pre_len + n_fft + cp
        samples, no accepted candidate, or a body that has not fully arrived), else a BurstStep:
        a packet with consume_to = start + pre_len + the body's samples, or an RxError with
        consume_to = min(start + pre_len, len). NaN and infinities are handled as the reference
        handles them here, on the host only."""
        iq = _ofdm_arr(iq, np.complex64, "iq")
        pre_len = self.preamble.total_len
        if iq.size < pre_len + self.n_fft + self.cp_len:
            return None
        best = earliest_accepted(ofdm_sync(iq, self.fs, self.preamble, 0, iq.size), self.score_threshold, pre_len)
        if best is None:
            return None
        spacing = np.float32(self.fs) / np.float32(self.n_fft)
        total = np.float32(best.cfo_hz + np.float32(np.float32(best.integer_cfo_bins) * spacing))
        corrected = ofdm_rotate_block(np.ascontiguousarray(iq[best.start_sample:]), -total, self.fs)
        est = self._channel_host(corrected)
        if corrected.size < pre_len:
            return None
        got = self._body_host(corrected[pre_len:], est)
        if got is None:
            return None
        if isinstance(got, RxError):
            return BurstStep(None, got, min(best.start_sample + pre_len, iq.size), total, best.start_sample, best.score)
        packet, consumed, out, syms = got
        consume_to = best.start_sample + pre_len + consumed
        if consume_to > iq.size:
            return None
        return BurstStep(packet, None, consume_to, total, best.start_sample, best.score, out.inner_ok, out.outer_ok,
                         out.crc_ok, syms)


    def receive_frames(self, iq, stream=None, debug=False) -> dict:
        """receive for every row of iq (ncap, n) on the GPU: the earliest accepted frame of each
        capture. The launches: ofdm_sync_batch (metric, select, integer offset), the carrier
        correction of every capture from its accepted start, the equalizer weights from the
        corrected training symbols; then what decode_frames does, with the equalizer and the
        phase tracker between the demodulator and the LLRs and each row's own sample count in
        place of the row length. Per capture, numpy arrays: status (-1 need more, 0 decoded, else
        the RX_ERRORS code), start_sample (-1: nothing accepted), cfo_hz (the total offset
        corrected), sync_score, consume_to (as receive reports it; 0 with status -1), and
        decode_frames' fields (error is status with -1 as 0). debug=True adds corrected (ncap, n)
        and weights (ncap, n_fft) as they are on the device and symbols, per capture the payload's
        equalized symbols after the phase tracker (None where no payload was demodulated). The
        preamble must carry a training symbol, and decode_frames' limits hold (no TX low-pass,
        the interleavers it refuses). The input must be finite: NaN and infinities are handled
        as the reference handles them by receive, on the host, only. numpy or a contiguous torch
        CUDA tensor, queued on torch's current stream or on stream."""
        import torch

        self._device_ok()
        if self.preamble.training is None:
            raise ValueError("receive_frames needs a training symbol in the preamble (receive takes either)")
        if not _is_torch(iq):
            if not isinstance(iq, np.ndarray) or iq.dtype != np.complex64 or iq.ndim != 2:
                raise ValueError("iq: expected a 2-D complex64 array")
            out = self.receive_frames(torch.from_numpy(np.ascontiguousarray(iq)).cuda(), stream, debug)
            if debug:
                if stream is not None:
                    torch.cuda.synchronize()
                out["corrected"], out["weights"] = out["corrected"].cpu().numpy(), out["weights"].cpu().numpy()
            return out
        if not iq.is_cuda or not iq.is_contiguous() or iq.dtype != torch.complex64 or iq.dim() != 2:
            raise ValueError("iq: expected a contiguous 2-D complex64 CUDA tensor")
        ns, n = int(iq.shape[0]), int(iq.shape[1])
        pre, pre_len = self.preamble, self.preamble.total_len
        out = {"status": np.full(ns, -1, np.int64), "start_sample": np.full(ns, -1, np.int64),
               "cfo_hz": np.zeros(ns, np.float32), "sync_score": np.zeros(ns, np.float32), "consume_to": np.zeros(ns, np.int64)}
        for k in ("error", "mcs_index", "sequence_num", "flags", "payload_len"):
            out[k] = np.zeros(ns, np.int64)
        for k in ("inner_ok", "outer_ok", "crc_ok"):
            out[k] = np.zeros(ns, bool)
        out["payloads"] = [np.zeros(0, np.uint8) for _ in range(ns)]
        if debug:
            out["symbols"] = [None] * ns
        pc = _preamble_c(pre)
        if ns == 0 or n < pre_len + self.n_fft + self.cp_len or \
                not _L.orion_ofdm_sync_offsets(n, float(self.fs), C.byref(pc), 0, n):
            if debug:
                out["corrected"] = torch.zeros((ns, n), dtype=torch.complex64, device=iq.device)
                out["weights"] = torch.zeros((ns, self.n_fft), dtype=torch.complex64, device=iq.device)
            return out
        sptr = SyncEngine._stream(iq, stream)
        with _TorchOn(iq, stream):
            sync = ofdm_sync_batch(iq, self.fs, pre, 0, n, self.score_threshold, stream)
            rows = torch.empty((ns, n), dtype=torch.complex64, device=iq.device)
            avail = torch.empty(ns, dtype=torch.int32, device=iq.device)
            total = torch.empty(ns, dtype=torch.float32, device=iq.device)
            weights = torch.empty((ns, self.n_fft), dtype=torch.complex64, device=iq.device)
            oc = _SyncOutC(**{k: sync["accepted_integer_cfo_bins" if k == "accepted_bins" else k].data_ptr()
                              for k, _, _ in _SYNC_BATCH_KEYS})
            h = _acquire_handle(pc)
            _arg_check(_L.orion_ofdm_acquire_correct_device(h, iq.data_ptr(), ns, n, float(self.fs), self.n_fft, C.byref(oc),
                                                            rows.data_ptr(), avail.data_ptr(), total.data_ptr(), sptr))
            _arg_check(_L.orion_ofdm_acquire_weights_device(h, rows.data_ptr(), ns, n, self._window_start(),
                                                            weights.data_ptr(), sptr))
            kept = []

            def llr_of(constellation, block, idx):
                dem = self.demod(constellation)
                raw = ofdm_demodulate_batch(dem, block, bits=False, llr=False, stream=stream)[0]
                w = weights if idx is None else weights.index_select(0, idx).contiguous()
                syms, llr = dem.equalize_track(raw, w, block.shape[1] // self.sps, stream=stream)
                if idx is not None and debug:
                    kept.append((idx, syms))
                return llr

            res, incomplete = self._decode_rows(rows[:, pre_len:], stream, llr_of, torch.clamp(avail - pre_len, min=0))
            if stream is not None:
                torch.cuda.current_stream(iq.device).synchronize()
            facts = torch.stack([sync["accepted_start"].to(torch.float64), total.to(torch.float64),
                                 sync["accepted_score"].to(torch.float64)], dim=1).cpu().numpy()
        start = facts[:, 0].astype(np.int64)
        found = start >= 0
        out["start_sample"] = start
        out["cfo_hz"], out["sync_score"] = facts[:, 1].astype(np.float32), facts[:, 2].astype(np.float32)
        done = found & ~incomplete
        for k in ("error", "mcs_index", "sequence_num", "flags", "payload_len", "inner_ok", "outer_ok", "crc_ok"):
            out[k][done] = res[k][done]
        out["status"][done] = res["error"][done]
        failed = done & (res["error"] != 0)
        out["consume_to"][failed] = np.minimum(start[failed] + pre_len, n)
        good = done & (res["error"] == 0)
        for mi, plen in {(int(a), int(b)) for a, b in zip(res["mcs_index"][good], res["payload_len"][good])}:
            mcs = self.mcs_table.get(mi)
            n_sym = self.payload_symbols(mcs, block_plan(plen, self.scheme(mcs)))
            sel = good & (res["mcs_index"] == mi) & (res["payload_len"] == plen)
            out["consume_to"][sel] = start[sel] + pre_len + (self.header_symbols + n_sym) * self.sps
        for c in np.flatnonzero(good):
            out["payloads"][c] = res["payloads"][c]
        if debug:
            out["corrected"], out["weights"] = rows, weights
            for idx, syms in kept:
                sy = syms.cpu().numpy()
                for j, c in enumerate(idx.cpu().numpy()):
                    out["symbols"][int(c)] = sy[j].reshape(-1, self.n_data)
        return out


class OfdmFrameStreamDemod:
    """OfdmFrameStreamDemod (demodulate/ofdm_frame.rs:1280-1460) on the host: a sample buffer
    drained front to back by OfdmBurstDemod.receive. feed and flush return the BurstSteps that
    completed, in order; every step's consume_to samples leave the buffer. evm_db, the error
    rates, the channel estimate and the probe of the reference are not built."""

    def __init__(self, cfg, mcs_table, preamble):
        self._demod = OfdmBurstDemod(cfg, mcs_table, preamble)
        self._buf = np.zeros(0, np.complex64)

    def with_score_threshold(self, t) -> "OfdmFrameStreamDemod":
        self._demod.score_threshold = float(t)
        return self

    def __len__(self):
        return int(self._buf.size)

    def len(self) -> int:
        return int(self._buf.size)

    def is_empty(self) -> bool:
        return self._buf.size == 0

    def clear(self):
        self._buf = np.zeros(0, np.complex64)

    def feed(self, iq) -> list:
        self._buf = np.concatenate([self._buf, _ofdm_arr(iq, np.complex64, "iq")])
        return self.flush()

    def flush(self) -> list:
        out = []
        while True:
            step = self._demod.receive(self._buf)
            if step is None:
                return out
            self._buf = np.ascontiguousarray(self._buf[step.consume_to:])
            out.append(step)


# ---- the DVB-T 2K frame: Figure-9a constellation, the four-phase pilot / TPS grid, the TPS word,
# guard-interval acquisition, DvbTFrameMod / DvbTFrameDemod (src/waveform/dvb_t.rs, dvb_t_tps.rs,
# src/sync/dvb_t_gi_sync.rs, src/modulate/dvb_t_frame.rs, src/demodulate/dvb_t_frame.rs) ----
class _GiOutC(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("start", "found", "score", "cfo_hz", "gamma", "phi", "metric", "gamma_all",
                                          "phi_all")]


def _dvbt_sigs():
    vp, sz, f, i = C.c_void_p, C.c_size_t, C.c_float, C.c_int
    pi, psz = C.POINTER(C.c_int), C.POINTER(C.c_size_t)
    sig = {
        "orion_dvbt_constants": (i, [vp, vp, vp, vp, vp]),
        "orion_dvbt_boosted_pilot_value": (f, [C.c_uint8]),
        "orion_dvbt_phase": (i, [i, vp, vp, vp, psz, vp, vp, psz, vp]),
        "orion_dvbt_map_host": (i, [vp, sz, sz, vp]), "orion_dvbt_demap_host": (i, [vp, sz, sz, vp]),
        "orion_dvbt_llr_host": (i, [vp, sz, sz, vp]),
        "orion_dvbt_tps_bch_encode": (i, [vp, vp]), "orion_dvbt_tps_bch_decode": (i, [vp, vp, pi]),
        "orion_dvbt_tps_pack": (i, [vp, vp]), "orion_dvbt_tps_unpack": (i, [vp, vp, pi]),
        "orion_dvbt_tps_encode_host": (i, [vp, sz, vp]), "orion_dvbt_tps_decide_host": (i, [vp, sz, vp, psz]),
        "orion_dvbt_gi_sync_host": (i, [vp, sz, sz, sz, f, sz, f, sz, f, C.POINTER(C.c_int64), vp, pi, vp]),
        "orion_dvbt_integer_cfo_host": (i, [vp, sz, sz, i, C.POINTER(C.c_int32), C.POINTER(f), pi]),
        "orion_dvbt_mod_symbols_host": (i, [vp, sz, sz, sz, vp, sz, sz, vp]),
        "orion_dvbt_demod_symbols_host": (i, [vp, sz, sz, sz, sz, vp, vp, vp]),
        "orion_dvbt_mod_symbols_device": (i, [vp, sz, sz, vp, vp, sz, sz, sz, sz, vp, vp]),
        "orion_dvbt_gi_sync_batch_device": (i, [vp, sz, sz, sz, sz, f, sz, f, sz, f, C.POINTER(_GiOutC), vp]),
        "orion_dvbt_demod_symbols_device": (i, [vp, sz, sz, vp, vp, sz, sz, sz, sz, vp, vp, vp, vp]),
        "orion_dvbt_tps_decode_device": (i, [vp, sz, sz, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(_L, name)
        fn.restype = res
        fn.argtypes = args


_dvbt_sigs()
DVB_T_N_FFT, DVB_T_KMAX, DVB_T_ACTIVE_CARRIERS, DVB_T_DATA_CARRIERS = 2048, 1704, 1705, 1512
DVB_T_SCATTERED_PHASES, DVB_T_SCATTERED_PILOT_SPACING, DVB_T_MAX_RX_WINDOW_BACKOFF = 4, 12, 85
TPS_CODEWORD_BITS, TPS_INFO_BITS, TPS_PARITY_BITS, TPS_CARRIER_COUNT, TPS_SYMBOLS_PER_FRAME = 67, 53, 14, 17, 68
TPS_SYNC_WORD_13, TPS_SYNC_WORD_24 = 0x35EE, 0xCA11
DVB_T_GUARDS = {"1/32": 0, "1/16": 1, "1/8": 2, "1/4": 3}
DVB_T_RX_ERRORS = {"acquisition": 1, "incomplete": 2, "tps_decode": 3, "payload_decode": 4}
_DVBT_ORDERS = {"qpsk": 1, "qam16": 2, "qam64": 3}
INTEGER_CFO_ACCUM_SYMBOLS, INTEGER_CFO_MAX_BINS = 8, 32
__all__ += ["DVB_T_N_FFT", "DVB_T_KMAX", "DVB_T_ACTIVE_CARRIERS", "DVB_T_DATA_CARRIERS", "DVB_T_SCATTERED_PHASES",
            "DVB_T_SCATTERED_PILOT_SPACING", "DVB_T_MAX_RX_WINDOW_BACKOFF", "TPS_CODEWORD_BITS", "TPS_INFO_BITS",
            "TPS_PARITY_BITS", "TPS_CARRIER_COUNT", "TPS_SYMBOLS_PER_FRAME", "TPS_SYNC_WORD_13", "TPS_SYNC_WORD_24",
            "DVB_T_GUARDS", "DVB_T_RX_ERRORS", "DVB_T_CONTINUAL_PILOTS_2K", "DVB_T_TPS_CARRIERS_2K", "wk_prbs",
            "boosted_pilot_value", "dvb_t_cp_len_2k", "scattered_pilot_indices", "tps_carrier_bins",
            "continual_pilot_bins", "dvb_t_2k_plans", "dvb_t_map_symbol", "dvb_t_demap_symbol", "dvb_t_soft_llr",
            "tps_bch_encode", "tps_bch_decode", "TpsWord", "TpsEncoder", "TpsDecoder", "GiSyncConfig", "GiSyncResult",
            "dvb_t_gi_sync", "dvb_t_gi_sync_with", "dvb_t_gi_refine", "dvb_t_gi_metric", "dvb_t_integer_cfo",
            "dvb_t_mod_symbols", "dvb_t_demod_symbols", "dvb_t_mod_symbols_batch", "dvb_t_gi_sync_batch",
            "dvb_t_demod_symbols_batch", "dvb_t_tps_decode_batch", "DvbTFrameParams", "DvbTFrame", "DvbTFrameMod",
            "DvbTRxError", "DvbTRxFrame", "DvbTFrameDemod"]


def _dvbt_constants():
    cont, tps = np.zeros(45, np.uint32), np.zeros(17, np.uint32)
    cb, tb, wk = np.zeros(45, np.uint32), np.zeros(17, np.uint32), np.zeros(DVB_T_ACTIVE_CARRIERS, np.uint8)
    _check(_L.orion_dvbt_constants(cont.ctypes.data, tps.ctypes.data, cb.ctypes.data, tb.ctypes.data, wk.ctypes.data))
    return cont, tps, cb, tb, wk


def _dvbt_guard(guard) -> int:
    g = DVB_T_GUARDS.get(guard, guard)
    if g not in (0, 1, 2, 3):
        raise ValueError(f"guard: one of {list(DVB_T_GUARDS)}")
    return int(g)


def _dvbt_v(v) -> int:
    if v not in (2, 4, 6):
        raise ValueError("v: 2, 4 or 6 bits per carrier")
    return int(v)


def wk_prbs(n) -> np.ndarray:
    """wk_prbs (dvb_t.rs:390-402): the first n <= 1705 bits of the X^11 + X^2 + 1 reference sequence."""
    if not 0 <= int(n) <= DVB_T_ACTIVE_CARRIERS:
        raise ValueError("wk_prbs: at most 1705 bits (one per active carrier)")
    return _dvbt_constants()[4][:int(n)].copy()


def boosted_pilot_value(wk) -> np.complex64:
    """boosted_pilot_value (dvb_t.rs:408-410): (4/3) 2 (1/2 - w_k), imaginary part 0."""
    return np.complex64(_L.orion_dvbt_boosted_pilot_value(int(wk) & 0xff))


def dvb_t_cp_len_2k(guard) -> int:
    """GuardInterval::cp_len_2k: 64, 128, 256, 512."""
    return DVB_T_N_FFT >> (5 - _dvbt_guard(guard))


def scattered_pilot_indices(phase) -> np.ndarray:
    """scattered_pilot_indices (dvb_t.rs:439-444): the active carriers k = 3 (phase mod 4) + 12 p <= 1704."""
    return np.arange(3 * (int(phase) % 4), DVB_T_KMAX + 1, 12, dtype=np.int64)


def tps_carrier_bins() -> np.ndarray:
    return _dvbt_constants()[3].astype(np.int64)


def continual_pilot_bins() -> np.ndarray:
    return _dvbt_constants()[2].astype(np.int64)


DVB_T_CONTINUAL_PILOTS_2K = tuple(int(v) for v in _dvbt_constants()[0])
DVB_T_TPS_CARRIERS_2K = tuple(int(v) for v in _dvbt_constants()[1])


def dvb_t_2k_plans(guard) -> list:
    """dvb_t_2k_plans (dvb_t.rs:494-521) with ScatteredGridCycle's reference pilots (:559-569): a dict
    per phase: cp_len, data_bins (1512, active-carrier order), pilot_bins / pilot_values (every
    reserved carrier: continual, the phase's scattered, TPS, with its boosted value), ref_bins /
    ref_values (the channel references: the pilots minus the 17 TPS bins, sorted by transform
    bin) and role (2048: >= 0 the data index, -1 null, -2 / -3 a pilot + / -, -4 - j TPS carrier
    j). The library refuses to build its tables unless each phase has exactly 1512 data carriers."""
    cp, out = dvb_t_cp_len_2k(guard), []
    for p in range(4):
        db, pb, pv = np.zeros(1512, np.uint32), np.zeros(256, np.uint32), np.zeros(256, np.float32)
        rb, rv, role = np.zeros(256, np.uint32), np.zeros(256, np.float32), np.zeros(2048, np.int32)
        npil, nref = C.c_size_t(0), C.c_size_t(0)
        _arg_check(_L.orion_dvbt_phase(p, db.ctypes.data, pb.ctypes.data, pv.ctypes.data, C.byref(npil), rb.ctypes.data,
                                       rv.ctypes.data, C.byref(nref), role.ctypes.data))
        out.append({"cp_len": cp, "data_bins": db.astype(np.int64), "pilot_bins": pb[:npil.value].astype(np.int64),
                    "pilot_values": pv[:npil.value].astype(np.complex64), "ref_bins": rb[:nref.value].astype(np.int64),
                    "ref_values": rv[:nref.value].astype(np.complex64), "role": role})
    return out


def dvb_t_map_symbol(bits):
    """dvb_t_map_symbol (dvb_t.rs:157-182): v = 2, 4 or 6 bits, or (n, v) rows -> complex64; even
    bits on I, odd on Q, Figure 9a's Gray labels. None for another v, as the reference."""
    b = np.ascontiguousarray(bits, np.uint8)
    if b.shape[-1] not in (2, 4, 6) or b.ndim not in (1, 2):
        return None
    rows = b.reshape(-1, b.shape[-1])
    out = np.zeros(rows.shape[0], np.complex64)
    _arg_check(_L.orion_dvbt_map_host(rows.ctypes.data, rows.shape[0], rows.shape[1], out.ctypes.data))
    return out[0] if b.ndim == 1 else out


def _dvbt_syms(sym):
    one = np.ndim(sym) == 0
    return np.ascontiguousarray(sym, np.complex64).reshape(-1), one


def dvb_t_demap_symbol(sym, v):
    """dvb_t_demap_symbol (dvb_t.rs:187-216): the nearest point's bits, (v,) or (n, v) uint8."""
    if v not in (2, 4, 6):
        return None
    s, one = _dvbt_syms(sym)
    out = np.zeros((s.size, v), np.uint8)
    _arg_check(_L.orion_dvbt_demap_host(s.ctypes.data, s.size, v, out.ctypes.data))
    return out[0] if one else out


def dvb_t_soft_llr(sym, v):
    """dvb_t_soft_llr (dvb_t.rs:228-266): max-log LLRs in y0 .. y(v-1) order, positive = 0."""
    if v not in (2, 4, 6):
        return None
    s, one = _dvbt_syms(sym)
    out = np.zeros((s.size, v), np.float32)
    _arg_check(_L.orion_dvbt_llr_host(s.ctypes.data, s.size, v, out.ctypes.data))
    return out[0] if one else out


def _dvbt_bits(x, n, what):
    b = np.ascontiguousarray(x, np.uint8)
    if b.shape != (n,):
        raise ValueError(f"{what}: {n} bits, one per element")
    return b


def tps_bch_encode(info) -> np.ndarray:
    """tps_bch_encode (dvb_t_tps.rs:109-118): 53 bits -> [info | 14 parity bits], generator 0x4377."""
    b, out = _dvbt_bits(info, TPS_INFO_BITS, "info"), np.zeros(TPS_CODEWORD_BITS, np.uint8)
    _check(_L.orion_dvbt_tps_bch_encode(b.ctypes.data, out.ctypes.data))
    return out


def tps_bch_decode(codeword):
    """tps_bch_decode (dvb_t_tps.rs:154-247): up to two errors corrected over GF(2^7) (0x89), the
    corrected word re-encoded as a check; the 53 information bits, or None."""
    b = np.ascontiguousarray(codeword, np.uint8)
    if b.shape != (TPS_CODEWORD_BITS,):
        return None
    out, ok = np.zeros(TPS_INFO_BITS, np.uint8), C.c_int(0)
    _check(_L.orion_dvbt_tps_bch_decode(b.ctypes.data, out.ctypes.data, C.byref(ok)))
    return out if ok.value else None


class TpsWord:
    """TpsWord (dvb_t_tps.rs:293-450): frame_number 0..3, constellation "qpsk" / "qam16" / "qam64",
    code_rate_hp "1/2" .. "7/8", guard "1/32" .. "1/4", cell_id one byte."""

    def __init__(self, frame_number, constellation, code_rate_hp, guard, cell_id):
        if constellation not in _DVBT_ORDERS:
            raise ValueError(f"constellation: one of {list(_DVBT_ORDERS)}")
        self.frame_number, self.constellation, self.code_rate_hp = int(frame_number), constellation, code_rate_hp
        self.guard, self.cell_id = {v: k for k, v in DVB_T_GUARDS.items()}[_dvbt_guard(guard)], int(cell_id)
        _fec_rate(code_rate_hp)

    def _fields(self):
        return np.array([self.frame_number & 3, _DVBT_ORDERS[self.constellation], _fec_rate(self.code_rate_hp),
                         DVB_T_GUARDS[self.guard], self.cell_id & 0xff], np.int32)

    @classmethod
    def _from_fields(cls, f):
        return cls(int(f[0]), {v: k for k, v in _DVBT_ORDERS.items()}[int(f[1])],
                   {v: k for k, v in FEC_RATES.items()}[int(f[2])], int(f[3]), int(f[4]))

    def pack(self) -> np.ndarray:
        """The 68 bits s0 .. s67: s0 = 0, the sync word by frame parity, the fields, the BCH parity."""
        f, out = self._fields(), np.zeros(68, np.uint8)
        _arg_check(_L.orion_dvbt_tps_pack(f.ctypes.data, out.ctypes.data))
        return out

    @classmethod
    def unpack(cls, bits):
        """unpack (dvb_t_tps.rs:425-449): None for an uncorrectable word or a reserved constellation
        or rate code; s0 is ignored."""
        b = np.ascontiguousarray(bits, np.uint8)
        if b.shape != (68,):
            return None
        f, ok = np.zeros(5, np.int32), C.c_int(0)
        _check(_L.orion_dvbt_tps_unpack(b.ctypes.data, f.ctypes.data, C.byref(ok)))
        return cls._from_fields(f) if ok.value else None

    def astuple(self):
        return (self.frame_number, self.constellation, self.code_rate_hp, self.guard, self.cell_id)

    def __eq__(self, o):
        return isinstance(o, TpsWord) and self.astuple() == o.astuple()

    def __hash__(self):
        return hash(self.astuple())

    def __repr__(self):
        return "TpsWord(frame_number=%d, constellation=%r, code_rate_hp=%r, guard=%r, cell_id=%d)" % self.astuple()


class TpsEncoder:
    """TpsEncoder (dvb_t_tps.rs:491-538): DBPSK along the symbol axis from the w_k reference signs."""

    def __init__(self):
        self.reset()

    def reset(self):
        self._sign, self.symbol = np.float32(1.0), 0

    def next_symbol(self, bit) -> np.ndarray:
        if self.symbol > 0 and (int(bit) & 1):
            self._sign = -self._sign
        self.symbol += 1
        return (self._sign * _tps_reference_signs()).astype(np.complex64)


def _tps_reference_signs() -> np.ndarray:
    one = np.zeros(68, np.uint8)
    out = np.zeros(17, np.complex64)
    _check(_L.orion_dvbt_tps_encode_host(one.ctypes.data, 1, out.ctypes.data))
    return out.real.astype(np.float32)


class TpsDecoder:
    """TpsDecoder (dvb_t_tps.rs:546-614): bit l = (the 17 products cell conj(prev), real parts summed
    in carrier order) < 0, so a sum of exactly 0 gives 0; bit 0 is 0."""

    def __init__(self):
        self.reset()

    def reset(self):
        self._cells = []

    def feed_symbol(self, cells):
        c = np.ascontiguousarray(cells, np.complex64)
        if c.ndim != 1 or c.size < 17:
            raise ValueError("cells: the 17 TPS cells of one symbol")
        self._cells.append(c[:17].copy())

    def bits(self) -> np.ndarray:
        if not self._cells:
            return np.zeros(0, np.uint8)
        c = np.ascontiguousarray(np.stack(self._cells), np.complex64)
        out, n = np.zeros(68, np.uint8), C.c_size_t(0)
        _check(_L.orion_dvbt_tps_decide_host(c.ctypes.data, c.shape[0], out.ctypes.data, C.byref(n)))
        return out[:n.value]

    def is_complete(self) -> bool:
        return len(self._cells) >= 68

    def word(self):
        return TpsWord.unpack(self.bits()[:68]) if self.is_complete() else None


class GiSyncConfig:
    """GiSyncConfig (dvb_t_gi_sync.rs:57-127): rho weights the energy term of |gamma| - rho Phi,
    max_symbols bounds the coherent accumulation, origin_score_ratio guards the origin unwrap."""

    def __init__(self, rho=0.95, max_symbols=4, origin_score_ratio=0.5):
        self.rho, self.max_symbols, self.origin_score_ratio = float(rho), int(max_symbols), float(origin_score_ratio)
        if self.max_symbols < 0:
            raise ValueError("max_symbols is not negative")


class GiSyncResult:
    """GiSyncResult (dvb_t_gi_sync.rs:132-143) with the winning offset's sums: start_sample, cfo_hz,
    score, gamma (complex64) and phi (float32)."""

    def __init__(self, start_sample, cfo_hz, score, gamma=0j, phi=0.0):
        self.start_sample, self.cfo_hz, self.score = int(start_sample), np.float32(cfo_hz), np.float32(score)
        self.gamma, self.phi = np.complex64(gamma), np.float32(phi)

    def __repr__(self):
        return f"GiSyncResult(start_sample={self.start_sample}, cfo_hz={self.cfo_hz}, score={self.score})"


def _gi_sync_host(iq, n_fft, cp_len, fs, search_len, cfg, metric=False):
    iq = _ofdm_arr(iq, np.complex64, "iq")
    cfg = cfg if cfg is not None else GiSyncConfig()
    if min(int(n_fft), int(cp_len), int(search_len)) < 0:
        raise ValueError("n_fft, cp_len and search_len are not negative")
    start, found, out = C.c_int64(0), C.c_int(0), np.zeros(5, np.float32)
    m = np.zeros(int(search_len), np.float32) if metric else None
    _arg_check(_L.orion_dvbt_gi_sync_host(iq.ctypes.data, iq.size, int(n_fft), int(cp_len), float(fs), int(search_len),
                                          cfg.rho, cfg.max_symbols, cfg.origin_score_ratio, C.byref(start),
                                          out.ctypes.data, C.byref(found), m.ctypes.data if metric else None))
    res = GiSyncResult(start.value, out[0], out[1], complex(out[2], out[3]), out[4]) if found.value else None
    return (res, m if found.value else None) if metric else res


def dvb_t_gi_sync_with(iq, n_fft, cp_len, fs, search_len, cfg=None):
    """dvb_t_gi_sync_with (dvb_t_gi_sync.rs:169-286) on the host: gamma and Phi summed sequentially
    over k, then over up to max_symbols symbols that fit, Phi halved after the sum; the metric
    |gamma| - rho Phi; the argmax by total_cmp with the last of equal maxima; the two-condition
    origin unwrap on single-symbol scores; score = min(|gamma| / Phi, 1); cfo_hz = -atan2(gamma.im,
    gamma.re) fs / (TAU n_fft). |gamma| is the float32 rounding of the float64 square root of the
    float64 sum of the two exact squares. None where the reference returns None."""
    return _gi_sync_host(iq, n_fft, cp_len, fs, search_len, cfg)


def dvb_t_gi_sync(iq, n_fft, cp_len, fs, search_len):
    return _gi_sync_host(iq, n_fft, cp_len, fs, search_len, None)


def dvb_t_gi_metric(iq, n_fft, cp_len, fs, search_len, cfg=None):
    """(result, metric float32 (search_len,)) of dvb_t_gi_sync_with: the ranked metric per offset."""
    return _gi_sync_host(iq, n_fft, cp_len, fs, search_len, cfg, metric=True)


def dvb_t_gi_refine(iq, n_fft, cp_len, fs, coarse, radius, cfg=None):
    """dvb_t_gi_refine_with (dvb_t_gi_sync.rs:319-338): a plain argmax within coarse +- radius."""
    iq = _ofdm_arr(iq, np.complex64, "iq")
    cfg = cfg if cfg is not None else GiSyncConfig()
    start = max(int(coarse) - int(radius), 0)
    if start > iq.size:
        return None
    sub = np.ascontiguousarray(iq[start:])
    r = _gi_sync_host(sub, n_fft, cp_len, fs, min(2 * int(radius) + 1, sub.size), GiSyncConfig(cfg.rho, cfg.max_symbols, 0.0))
    if r is not None:
        r.start_sample += start
    return r


def dvb_t_integer_cfo(freq, n_fft, max_bins):
    """dvb_t_integer_cfo (dvb_t_gi_sync.rs:380-417): (bins, confidence) of the shift in -max_bins ..
    max_bins with the most energy at the 45 continual-pilot bins (the first of equal maxima), or None."""
    fq = _ofdm_arr(freq, np.complex64, "freq")
    bins, conf, found = C.c_int32(0), C.c_float(0.0), C.c_int(0)
    _arg_check(_L.orion_dvbt_integer_cfo_host(fq.ctypes.data, fq.size, int(n_fft), int(max_bins), C.byref(bins),
                                              C.byref(conf), C.byref(found)))
    return (int(bins.value), np.float32(conf.value)) if found.value else None


def dvb_t_mod_symbols(coded_bits, v, cp_len, tps_bits, n_symbols, roll_off=0) -> np.ndarray:
    """The frame modulator from the coded bits on (modulate/dvb_t_frame.rs:213-261), host: Figure-9a
    mapping through the four-phase grid, the TPS cells, inverse transform, cyclic prefix, window.
    A data carrier whose v bits lie past the coded bits is zero."""
    b = np.ascontiguousarray(coded_bits, np.uint8).reshape(-1)
    t = _dvbt_bits(tps_bits, 68, "tps_bits")
    out = np.zeros(int(n_symbols) * (DVB_T_N_FFT + int(cp_len)), np.complex64)
    _arg_check(_L.orion_dvbt_mod_symbols_host(b.ctypes.data, b.size, _dvbt_v(v), int(cp_len), t.ctypes.data, int(n_symbols),
                                              int(roll_off), out.ctypes.data))
    return out


def dvb_t_demod_symbols(iq, n_symbols, cp_len, backoff, v, syms=False):
    """The frame demodulator's symbol loop (demodulate/dvb_t_frame.rs:497-583) from an acquired
    start, host: (llr float32 (n_symbols, 1512 v), cells complex64 (n_symbols, 17)[, equalized
    data symbols complex64 (n_symbols, 1512)])."""
    iq = _ofdm_arr(iq, np.complex64, "iq")
    ns, sps = int(n_symbols), DVB_T_N_FFT + int(cp_len)
    if iq.size < ns * sps:
        raise ValueError("iq: n_symbols whole symbols")
    llr, cells = np.zeros((ns, 1512 * _dvbt_v(v)), np.float32), np.zeros((ns, 17), np.complex64)
    eq = np.zeros((ns, 1512), np.complex64) if syms else None
    _arg_check(_L.orion_dvbt_demod_symbols_host(iq.ctypes.data, ns, int(cp_len), int(backoff), v, llr.ctypes.data,
                                                cells.ctypes.data, eq.ctypes.data if syms else None))
    return (llr, cells, eq) if syms else (llr, cells)


def _dvbt_cuda(x, dtype, dims, what):
    import torch

    if not _is_torch(x) or not x.is_cuda or not x.is_contiguous() or x.dtype != getattr(torch, dtype) or x.dim() != dims:
        raise ValueError(f"{what}: a contiguous {dims}-D {dtype} CUDA tensor")
    return x


def _dvbt_numpy_in(x, dtype, what):
    import torch

    if not isinstance(x, np.ndarray) or x.dtype != dtype or x.ndim != 2:
        raise ValueError(f"{what}: expected a 2-D {np.dtype(dtype).name} array")
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _dvbt_tps_words(tps_bits, frames, device):
    """(frames, 68) bits -> (frames, 3) int32 on the device, bit l of a row's 96 the bit s_l."""
    import torch

    t = np.ascontiguousarray(tps_bits, np.uint8)
    if t.shape != (frames, 68):
        raise ValueError("tps_bits: (frames, 68) bits")
    padded = np.zeros((frames, 96), np.uint8)
    padded[:, :68] = t & 1
    words = np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(frames, 3)
    return torch.from_numpy(words.view(np.int32).copy()).to(device)


def dvb_t_mod_symbols_batch(coded_bits, v, cp_len, tps_bits, n_symbols, roll_off=0, nbits=None, stream=None):
    """dvb_t_mod_symbols for every row of coded_bits uint8 (frames, row_bits) on the GPU, one
    workgroup per (frame, symbol): tps_bits (frames, 68) host bits (every frame its own word),
    nbits (frames,) the bits a row really holds (default row_bits) -> complex64 (frames, n_symbols
    (2048 + cp_len)), row k the host's bits. numpy in -> numpy out; a contiguous torch CUDA tensor
    stays resident, queued on torch's current stream or on stream."""
    import torch

    if not _is_torch(coded_bits):
        out = dvb_t_mod_symbols_batch(_dvbt_numpy_in(coded_bits, np.uint8, "coded_bits"), v, cp_len, tps_bits, n_symbols,
                                      roll_off, nbits, stream)
        if stream is not None:
            torch.cuda.synchronize()
        return out.cpu().numpy()
    b = _dvbt_cuda(coded_bits, "uint8", 2, "coded_bits")
    frames, row_bits, ns = int(b.shape[0]), int(b.shape[1]), int(n_symbols)
    with _TorchOn(b, stream):
        words = _dvbt_tps_words(tps_bits, frames, b.device)
        nb = None
        if nbits is not None:
            nb = np.ascontiguousarray(nbits, np.int64)
            if nb.shape != (frames,) or nb.min(initial=0) < 0 or nb.max(initial=0) > row_bits:
                raise ValueError("nbits: (frames,) counts within a row")
            nb = torch.from_numpy(nb.astype(np.int32)).to(b.device)
        out = torch.zeros((frames, ns * (DVB_T_N_FFT + int(cp_len))), dtype=torch.complex64, device=b.device)
        _arg_check(_L.orion_dvbt_mod_symbols_device(b.data_ptr(), frames, row_bits, nb.data_ptr() if nb is not None else None,
                                                    words.data_ptr(), _dvbt_v(v), int(cp_len), ns, int(roll_off),
                                                    out.data_ptr(), SyncEngine._stream(b, stream)))
    return out


_GI_BATCH_KEYS = (("start", "int32", 1), ("found", "int32", 1), ("score", "float32", 1), ("cfo_hz", "float32", 1),
                  ("gamma", "complex64", 1), ("phi", "float32", 1), ("metric", "float32", None),
                  ("gamma_all", "complex64", None), ("phi_all", "float32", None))


def dvb_t_gi_sync_batch(iq, n_fft, cp_len, fs, search_len, cfg=None, stream=None) -> dict:
    """dvb_t_gi_sync_with for every row of iq (ncap, n) on the GPU, one independent search per
    capture. Returns per capture start int32, found int32 (0 where the host returns None: the
    capture is too short), score, cfo_hz, phi float32 and gamma complex64, and per offset metric,
    phi_all float32 and gamma_all complex64 (ncap, search_len). Everything but cfo_hz carries the
    host's bits; cfo_hz is the device's atan2f. numpy in -> numpy out; a contiguous
    2-D complex64 CUDA tensor stays resident, queued on torch's current stream or on stream."""
    import torch

    if not _is_torch(iq):
        out = dvb_t_gi_sync_batch(_dvbt_numpy_in(iq, np.complex64, "iq"), n_fft, cp_len, fs, search_len, cfg, stream)
        if stream is not None:
            torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}
    iq = _dvbt_cuda(iq, "complex64", 2, "iq")
    cfg = cfg if cfg is not None else GiSyncConfig()
    ncap, n, sl = int(iq.shape[0]), int(iq.shape[1]), int(search_len)
    if min(int(n_fft), int(cp_len), sl) < 0:
        raise ValueError("n_fft, cp_len and search_len are not negative")
    with _TorchOn(iq, stream):
        out = {}
        for k, dt, w in _GI_BATCH_KEYS:
            out[k] = torch.zeros((ncap,) if w == 1 else (ncap, max(sl, 1)), dtype=getattr(torch, dt), device=iq.device)
        if ncap:
            oc = _GiOutC(*[out[k].data_ptr() for k, _, _ in _GI_BATCH_KEYS])
            _arg_check(_L.orion_dvbt_gi_sync_batch_device(iq.data_ptr(), ncap, n, int(n_fft), int(cp_len), float(fs), sl,
                                                          cfg.rho, cfg.max_symbols, cfg.origin_score_ratio, C.byref(oc),
                                                          SyncEngine._stream(iq, stream)))
        for k in ("metric", "gamma_all", "phi_all"):
            out[k] = out[k][:, :sl]
    return out


def dvb_t_demod_symbols_batch(iq, start, found, n_symbols, cp_len, backoff, v, syms=False, stream=None) -> dict:
    """dvb_t_demod_symbols for every row of iq (ncap, n) on the GPU from start[c] (int32 (ncap,), as
    dvb_t_gi_sync_batch gives it): llr float32 (ncap, n_symbols, 1512 v), cells complex64 (ncap,
    n_symbols, 17) and with syms the equalized data symbols (ncap, n_symbols, 1512), each the
    host's bits; zeros for a capture with found[c] == 0 or whose n_symbols symbols do not fit."""
    import torch

    if not _is_torch(iq):
        dev = _dvbt_numpy_in(iq, np.complex64, "iq")
        st = torch.from_numpy(np.ascontiguousarray(start, np.int32)).to(dev.device)
        fd = torch.from_numpy(np.ascontiguousarray(found, np.int32)).to(dev.device)
        out = dvb_t_demod_symbols_batch(dev, st, fd, n_symbols, cp_len, backoff, v, syms, stream)
        if stream is not None:
            torch.cuda.synchronize()
        return {k: x.cpu().numpy() for k, x in out.items()}
    iq = _dvbt_cuda(iq, "complex64", 2, "iq")
    ncap, n, ns = int(iq.shape[0]), int(iq.shape[1]), int(n_symbols)
    st, fd = _dvbt_cuda(start, "int32", 1, "start"), _dvbt_cuda(found, "int32", 1, "found")
    if int(st.shape[0]) != ncap or int(fd.shape[0]) != ncap or int(backoff) < 0:
        raise ValueError("start, found: one entry per capture; backoff is not negative")
    with _TorchOn(iq, stream):
        out = {"llr": torch.zeros((ncap, ns, 1512 * _dvbt_v(v)), dtype=torch.float32, device=iq.device),
               "cells": torch.zeros((ncap, ns, 17), dtype=torch.complex64, device=iq.device)}
        if syms:
            out["syms"] = torch.zeros((ncap, ns, 1512), dtype=torch.complex64, device=iq.device)
        _arg_check(_L.orion_dvbt_demod_symbols_device(iq.data_ptr(), ncap, n, st.data_ptr(), fd.data_ptr(), ns, int(cp_len),
                                                      int(backoff), v, out["llr"].data_ptr(), out["cells"].data_ptr(),
                                                      out["syms"].data_ptr() if syms else None,
                                                      SyncEngine._stream(iq, stream)))
    return out


def dvb_t_tps_decode_batch(cells, stream=None) -> dict:
    """TpsDecoder + TpsWord::unpack over the first 68 symbols of cells complex64 (frames, n_symbols,
    17) on the GPU, one wave per frame: fields int32 (frames, 5) (frame_number, constellation,
    code rate, guard, cell_id as the library's codes) and status int32 (frames,): 0 decoded, 1 not
    (fewer than 68 symbols, an uncorrectable word, a reserved code)."""
    import torch

    if not _is_torch(cells):
        c = np.ascontiguousarray(cells, np.complex64)
        if c.ndim != 3 or c.shape[2] != 17:
            raise ValueError("cells: (frames, n_symbols, 17) complex64")
        out = dvb_t_tps_decode_batch(torch.from_numpy(c).cuda(), stream)
        if stream is not None:
            torch.cuda.synchronize()
        return {k: x.cpu().numpy() for k, x in out.items()}
    c = _dvbt_cuda(cells, "complex64", 3, "cells")
    if int(c.shape[2]) != 17:
        raise ValueError("cells: (frames, n_symbols, 17) complex64")
    frames = int(c.shape[0])
    with _TorchOn(c, stream):
        out = {"fields": torch.zeros((frames, 5), dtype=torch.int32, device=c.device),
               "status": torch.ones((frames,), dtype=torch.int32, device=c.device)}
        _arg_check(_L.orion_dvbt_tps_decode_device(c.data_ptr(), frames, int(c.shape[1]), out["fields"].data_ptr(),
                                                   out["status"].data_ptr(), SyncEngine._stream(c, stream)))
    return out


def _dvbt_fs() -> float:
    """dvb_t_fs_for_bandwidth(1 MHz) (dvb_t.rs:726-728), the frame classes' sample rate."""
    return float(np.float32(1_000_000.0) * np.float32(DVB_T_N_FFT) / np.float32(DVB_T_ACTIVE_CARRIERS))


class DvbTFrameParams:
    """DvbTFrameParams (dvb_t.rs:898-953): guard "1/32" .. "1/4", constellation "qpsk" / "qam16" /
    "qam64", code_rate "1/2" .. "7/8", frame_number 0..3 and the cell-id byte."""

    def __init__(self, guard="1/32", constellation="qpsk", code_rate="1/2", frame_number=0, cell_id=0):
        self._tps = TpsWord(frame_number, constellation, code_rate, guard, cell_id)
        if not 0 <= int(frame_number) <= 3 or not 0 <= int(cell_id) <= 255:
            raise ValueError("frame_number 0..3, cell_id 0..255")
        self.guard, self.constellation, self.code_rate = self._tps.guard, constellation, code_rate
        self.frame_number, self.cell_id = int(frame_number), int(cell_id)
        self.cp_len, self.bits_per_carrier = dvb_t_cp_len_2k(guard), 2 * _DVBT_ORDERS[constellation]
        self.fs = _dvbt_fs()

    def tps_word(self) -> TpsWord:
        return self._tps

    def scheme(self) -> FrameScheme:
        """The DVB coding chain: no CRC, RS(204,188), the K = 7 code at the frame's rate, Forney
        I = 12 / M = 17, no scrambler (the TS energy dispersal runs outside the chain)."""
        return FrameScheme(crc="none", outer=("rs", 204, 16), inner=("conv", self.code_rate, "dvb_k7"),
                           outer_interleaver=("forney", 12, 17), scrambler=None)

    def with_frame(self, frame_number, cell_id) -> "DvbTFrameParams":
        return DvbTFrameParams(self.guard, self.constellation, self.code_rate, frame_number, cell_id)


class DvbTFrame:
    """DvbTFrame (modulate/dvb_t_frame.rs:47-55)."""

    def __init__(self, iq, n_symbols, samples_per_symbol):
        self.iq, self.n_symbols, self.samples_per_symbol = iq, int(n_symbols), int(samples_per_symbol)


class DvbTFrameMod:
    """DvbTFrameMod (modulate/dvb_t_frame.rs:61-277): a TS payload -> one preamble-less DVB-T frame.
    modulate is the library's host code; modulate_frames the same frames batched on the GPU."""

    def __init__(self, params):
        if not isinstance(params, DvbTFrameParams):
            raise ValueError("params: a DvbTFrameParams")
        self.params, self._roll, self._lowpass = params, 0, None

    def with_symbol_window(self, roll_off) -> "DvbTFrameMod":
        if int(roll_off) < 0 or int(roll_off) > 4095:
            raise ValueError("roll_off: 0 .. 4095 samples")
        self._roll = int(roll_off)
        return self

    def with_tx_lowpass(self, lowpass) -> "DvbTFrameMod":
        if not isinstance(lowpass, TxLowpass):
            raise ValueError("lowpass: a TxLowpass")
        self._lowpass = lowpass
        return self

    @staticmethod
    def tx_lowpass_for_2k(num_taps, stopband_db) -> TxLowpass:
        return TxLowpass.for_null_band(DVB_T_N_FFT, DVB_T_KMAX // 2, int(num_taps), float(stopband_db))

    def plan(self, payload_len):
        """(n_symbols, target_packets): max(payload symbols, 68), and the packets after null-packet
        stuffing, the fewest (at least the payload's) whose coded stream fills every carrier."""
        p, sch = self.params, self.params.scheme()
        per_sym = DVB_T_DATA_CARRIERS * p.bits_per_carrier
        n_real = max(1, -(-int(payload_len) // 187))
        n_symbols = max(symbols_for_coded_bits(DVB_T_DATA_CARRIERS, p.bits_per_carrier,
                                               block_plan(n_real * TS_PACKET_LEN, sch).coded_bits), TPS_SYMBOLS_PER_FRAME)
        target = n_real
        while block_plan(target * TS_PACKET_LEN, sch).coded_bits < n_symbols * per_sym:
            target += 1
        return n_symbols, target

    def _ts(self, payload, target) -> np.ndarray:
        return ts_energy_disperse(ts_stuff_null_packets(ts_packetize(payload), target))

    def modulate(self, payload) -> DvbTFrame:
        """modulate (modulate/dvb_t_frame.rs:147-276) on the host."""
        payload = _bytes_arg(payload, "payload")
        p = self.params
        n_symbols, target = self.plan(payload.size)
        coded = encode_chain(self._ts(payload, target), p.scheme(), 0)
        iq = dvb_t_mod_symbols(coded, p.bits_per_carrier, p.cp_len, p.tps_word().pack(), n_symbols, self._roll)
        if self._lowpass is not None:
            iq = self._lowpass.apply(iq)
        return DvbTFrame(iq, n_symbols, DVB_T_N_FFT + p.cp_len)

    def modulate_frames(self, payloads, frame_numbers=None, cell_ids=None, stream=None):
        """A batch of equal-length payloads on the GPU: uint8 (B, n) -> complex64 (B, n_symbols (2048
        + cp_len)), row k equal to modulate of payload k under frame_numbers[k] / cell_ids[k]
        (default: the parameters'). The TS adaptation (packets, null-packet stuffing, energy
        dispersal) runs on the host; then frame_encode_chain_batch and k_dvbt_mod. numpy in ->
        numpy out; a contiguous torch CUDA tensor stays resident, queued on torch's current stream
        or on stream. with_tx_lowpass is the host path's: ValueError here."""
        import torch

        if self._lowpass is not None:
            raise ValueError("modulate_frames: with_tx_lowpass is taken by modulate (the host path) only")
        if not _is_torch(payloads):
            p, _ = _fec2_arg(payloads, "payloads", "uint8", (2,))
            out = self.modulate_frames(torch.from_numpy(p).cuda(), frame_numbers, cell_ids, stream)
            if stream is not None:
                torch.cuda.synchronize()
            return out.cpu().numpy()
        pl, _ = _fec2_arg(payloads, "payloads", "uint8", (2,))
        par = self.params
        frames, n = int(pl.shape[0]), int(pl.shape[1])
        fn = np.full(frames, par.frame_number) if frame_numbers is None else np.asarray(frame_numbers, np.int64)
        ci = np.full(frames, par.cell_id) if cell_ids is None else np.asarray(cell_ids, np.int64)
        if fn.shape != (frames,) or ci.shape != (frames,):
            raise ValueError("frame_numbers, cell_ids: one entry per frame")
        n_symbols, target = self.plan(n)
        tps = np.stack([par.with_frame(int(a), int(b)).tps_word().pack() for a, b in zip(fn, ci)]) if frames else \
            np.zeros((0, 68), np.uint8)
        with _TorchOn(pl, stream):
            if stream is not None:
                torch.cuda.current_stream(pl.device).synchronize()
            host = pl.cpu().numpy()
            ts = np.stack([self._ts(row, target) for row in host]) if frames else np.zeros((0, target * 188), np.uint8)
            coded = frame_encode_chain_batch(torch.from_numpy(ts).to(pl.device), par.scheme(), stream=stream)
            return dvb_t_mod_symbols_batch(coded, par.bits_per_carrier, par.cp_len, tps, n_symbols, self._roll,
                                           stream=stream)


class DvbTRxError(Exception):
    """DvbTRxError (demodulate/dvb_t_frame.rs:213-222): kind "acquisition", "incomplete",
    "tps_decode" or "payload_decode"; code its DVB_T_RX_ERRORS number."""

    def __init__(self, kind):
        if kind not in DVB_T_RX_ERRORS:
            kind = {v: k for k, v in DVB_T_RX_ERRORS.items()}[int(kind)]
        super().__init__(kind)
        self.kind, self.code = kind, DVB_T_RX_ERRORS[kind]

    def __eq__(self, o):
        return (isinstance(o, DvbTRxError) and o.kind == self.kind) or o == self.kind

    def __hash__(self):
        return hash(self.kind)


class DvbTRxFrame:
    """DvbTRxFrame (demodulate/dvb_t_frame.rs:201-209): payload, tps (a TpsWord) and diagnostics, a
    dict with cfo_hz (total), sync_score, timing_offset_samples, integer_cfo_bins, outer_fec_ok,
    rs_corrected_bytes, and evm_db / channel_ber / inner_ber, which stay None."""

    def __init__(self, payload, tps, diagnostics):
        self.payload, self.tps, self.diagnostics = payload, tps, diagnostics


class DvbTFrameDemod:
    """DvbTFrameDemod (demodulate/dvb_t_frame.rs:239-768): IQ at an unknown start -> payload, TPS word
    and diagnostics. decode is the library's host code and raises DvbTRxError; decode_frames
    decodes a batch of captures on the GPU and reports the same outcome per capture."""

    def __init__(self, params):
        if not isinstance(params, DvbTFrameParams):
            raise ValueError("params: a DvbTFrameParams")
        self.params, self._icfo, self._backoff = params, False, 0

    def with_integer_cfo_correction(self, on=True) -> "DvbTFrameDemod":
        self._icfo = bool(on)
        return self

    def with_rx_window_backoff(self, backoff) -> "DvbTFrameDemod":
        if int(backoff) < 0:
            raise ValueError("backoff is not negative")
        self._backoff = int(backoff)
        return self

    def integer_cfo_correct(self, iq):
        """integer_cfo_correct (demodulate/dvb_t_frame.rs:342-394): (the rotated buffer or None, the
        estimate in bins or None); eight symbols' |X|^2 accumulated at the CP boundary, +-32 bins."""
        p = self.params
        sps = DVB_T_N_FFT + p.cp_len
        acq = dvb_t_gi_sync(iq, DVB_T_N_FFT, p.cp_len, p.fs, sps)
        if acq is None:
            return None, None
        accum = np.zeros(DVB_T_N_FFT, np.complex64)
        for s in range(INTEGER_CFO_ACCUM_SYMBOLS):
            off = acq.start_sample + s * sps
            if off + sps > iq.size:
                break
            f = fft_host(np.ascontiguousarray(iq[off + p.cp_len:off + sps]), DVB_T_N_FFT)
            e = (f.real * f.real + f.imag * f.imag).astype(np.float32)  # norm_sqr, one rounding per step
            accum = (accum.real + e).astype(np.float32).astype(np.complex64)
        est = dvb_t_integer_cfo(accum, DVB_T_N_FFT, INTEGER_CFO_MAX_BINS)
        if est is None:
            return None, None
        k = est[0]
        if k == 0:
            return None, 0
        return ofdm_rotate_block(iq, float(-np.float32(k) * np.float32(p.fs) / np.float32(DVB_T_N_FFT)), p.fs), k

    def decode(self, iq, n_symbols, payload_len) -> DvbTRxFrame:
        """decode (demodulate/dvb_t_frame.rs:406-767) on the host: TPS from the raw bins of the first
        68 symbols; the fractional CFO reported, not corrected; the payload's own packets (the
        prefix of the coded stream) decoded."""
        iq = _ofdm_arr(iq, np.complex64, "iq")
        p, n_symbols, payload_len = self.params, int(n_symbols), int(payload_len)
        sps = DVB_T_N_FFT + p.cp_len
        bins = None
        if self._icfo:
            rotated, bins = self.integer_cfo_correct(iq)
            iq = rotated if rotated is not None else iq
        acq = dvb_t_gi_sync(iq, DVB_T_N_FFT, p.cp_len, p.fs, sps)
        if acq is None:
            raise DvbTRxError("acquisition")
        start = acq.start_sample
        if iq.size < start + n_symbols * sps:
            raise DvbTRxError("incomplete")
        spacing = np.float32(p.fs) / np.float32(DVB_T_N_FFT)
        diag = {"cfo_hz": np.float32(acq.cfo_hz + np.float32(bins or 0) * spacing), "sync_score": acq.score,
                "timing_offset_samples": start, "integer_cfo_bins": bins, "evm_db": None, "channel_ber": None,
                "inner_ber": None, "outer_fec_ok": None, "rs_corrected_bytes": None}
        llr, cells = dvb_t_demod_symbols(np.ascontiguousarray(iq[start:start + n_symbols * sps]), n_symbols, p.cp_len,
                                         self._backoff, p.bits_per_carrier)
        dec = TpsDecoder()
        for c in cells[:68]:
            dec.feed_symbol(c)
        tps = dec.word()
        if tps is None:
            raise DvbTRxError("tps_decode")
        packets = max(1, -(-payload_len // 187))
        try:
            out = decode_chain(llr.reshape(-1), packets * TS_PACKET_LEN, p.scheme(), 0, "sum_product")
        except (RxError, ValueError):
            raise DvbTRxError("payload_decode") from None
        if not out.is_valid() or out.bytes.size < packets * TS_PACKET_LEN:
            raise DvbTRxError("payload_decode")
        diag["outer_fec_ok"], diag["rs_corrected_bytes"] = out.outer_ok, out.outer_corrected_bytes
        payload = ts_depacketize(ts_energy_disperse(out.bytes[:packets * TS_PACKET_LEN]))
        if payload is None:
            raise DvbTRxError("payload_decode")
        return DvbTRxFrame(payload[:payload_len], tps, diag)

    def decode_frames(self, iq, n_symbols, payload_len, stream=None) -> dict:
        """decode for every row of iq complex64 (B, L) on the GPU: k_gi_metric / k_gi_select,
        k_dvbt_demod, k_tps_decode, then frame_decode_chain_batch on each row's LLR prefix, and on
        the host the de-dispersal and depacketizing. Returns numpy arrays per capture: error (0 or
        the DvbTRxError code decode raises), frame_number, constellation, code_rate, guard, cell_id
        (the TPS fields as the library's codes; 0 where no word decoded), cfo_hz, sync_score,
        timing_offset_samples, integer_cfo_bins (-1: not measured), outer_fec_ok,
        rs_corrected_bytes, and payloads, a list of uint8 arrays (empty where error != 0). cfo_hz is
        the device's atan2f. with_integer_cfo_correction(True) is the host path's: ValueError."""
        import torch

        if self._icfo:
            raise ValueError("decode_frames: with_integer_cfo_correction is taken by decode (the host path) only")
        if not _is_torch(iq):
            return self.decode_frames(_dvbt_numpy_in(iq, np.complex64, "iq"), n_symbols, payload_len, stream)
        iq = _dvbt_cuda(iq, "complex64", 2, "iq")
        p, ns, payload_len = self.params, int(n_symbols), int(payload_len)
        B, L, sps = int(iq.shape[0]), int(iq.shape[1]), DVB_T_N_FFT + self.params.cp_len
        E = DVB_T_RX_ERRORS
        res = {k: np.zeros(B, np.int64) for k in ("error", "frame_number", "constellation", "code_rate", "guard", "cell_id",
                                                  "timing_offset_samples", "rs_corrected_bytes")}
        res.update({"cfo_hz": np.zeros(B, np.float32), "sync_score": np.zeros(B, np.float32),
                    "integer_cfo_bins": np.full(B, -1, np.int64), "outer_fec_ok": np.zeros(B, bool),
                    "payloads": [np.zeros(0, np.uint8) for _ in range(B)]})
        if B == 0:
            return res
        packets = max(1, -(-payload_len // 187))
        sch = p.scheme()
        with _TorchOn(iq, stream):
            acq = dvb_t_gi_sync_batch(iq, DVB_T_N_FFT, p.cp_len, p.fs, sps, stream=stream)
            dem = dvb_t_demod_symbols_batch(iq, acq["start"], acq["found"], ns, p.cp_len, self._backoff, p.bits_per_carrier,
                                            stream=stream)
            tps = dvb_t_tps_decode_batch(dem["cells"], stream=stream)
            need = block_plan(packets * TS_PACKET_LEN, sch).coded_bits
            llr = dem["llr"].reshape(B, -1)
            chain = None
            if int(llr.shape[1]) >= need:
                chain = frame_decode_chain_batch(llr, packets * TS_PACKET_LEN, sch, stream=stream)
            if stream is not None:
                torch.cuda.current_stream(iq.device).synchronize()
            head = torch.stack([acq["start"], acq["found"], tps["status"]], dim=1).cpu().numpy()
            fields = tps["fields"].cpu().numpy()
            res["cfo_hz"], res["sync_score"] = acq["cfo_hz"].cpu().numpy(), acq["score"].cpu().numpy()
            if chain is not None:
                ok = torch.stack([chain["valid"], chain["outer_ok"]], dim=1).cpu().numpy()
                corrected, pay = chain["corrected"].cpu().numpy(), chain["payload"].cpu().numpy()
        found = head[:, 1] != 0
        fits = found & (head[:, 0].astype(np.int64) + ns * sps <= L)
        tps_ok = fits & (head[:, 2] == 0)
        res["error"][~found] = E["acquisition"]
        res["error"][found & ~fits] = E["incomplete"]
        res["error"][fits & ~tps_ok] = E["tps_decode"]
        res["timing_offset_samples"][found] = head[found, 0]
        res["cfo_hz"][~found], res["sync_score"][~found] = 0.0, 0.0
        for j, key in enumerate(("frame_number", "constellation", "code_rate", "guard", "cell_id")):
            res[key][tps_ok] = fields[tps_ok, j]
        for c in np.flatnonzero(tps_ok):
            good = chain is not None and bool(ok[c, 0])
            payload = ts_depacketize(ts_energy_disperse(pay[c])) if good else None
            if payload is None:
                res["error"][c] = E["payload_decode"]
                continue
            res["outer_fec_ok"][c], res["rs_corrected_bytes"][c] = bool(ok[c, 1]), int(corrected[c])
            res["payloads"][c] = payload[:payload_len]
        return res
