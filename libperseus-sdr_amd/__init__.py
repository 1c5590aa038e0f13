"""libperseus-sdr_amd -- MI355X-native I/Q ingest + decimation path behind the
libperseus-sdr API.

This package is only a loader: the product is two C-ABI shared libraries built
from csrc/ (hand-written HIP for gfx950 + plain C host code):

  libperseus_ddc.so   include/perseus_ddc.h   kernels + stream pipeline
  libperseus-sdr.so   include/perseus-sdr.h   drop-in perseus_* callback API

Python (ctypes) is used by tests/ and bench.py to drive them; torch only
supplies device memory, streams and torch.distributed.  The hyphen in the
package name follows the reference repo's name, so import it with
importlib.import_module("libperseus-sdr_amd").

There is no CPU fallback anywhere in this package: if the HIP library is not
built, loading raises; if no GPU is present, compute entry points return
PDDC_ENODEV and the wrappers raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_HERE, "csrc")
# (tools/ab.sh points the ctypes binding at an alternative build of the kernel library -- same-box A/B measurements -- through
# PDDC_DDC_LIB instead of overwriting the product; nothing else reads it)
DDC_LIB = os.environ.get("PDDC_DDC_LIB") or os.path.join(_HERE, "libperseus_ddc.so")
SDR_LIB = os.path.join(_HERE, "libperseus-sdr.so")

PDDC_OK, PDDC_EINVAL, PDDC_ENODEV, PDDC_EHIP, PDDC_ENOMEM, PDDC_ECAPACITY, PDDC_ESTATE, PDDC_ECOMM = 0, -1, -2, -3, -4, -5, -6, -7
PDDC_COMM_ID_BYTES = 128
PDDC_F_MIX, PDDC_F_TAPS_FP16, PDDC_F_NO_FAST, PDDC_F_OUT_PACKED24 = 1, 2, 4, 8


class GangItem(C.Structure):
    """pddc_gang_item (include/perseus_ddc.h)"""
    _fields_ = [("pipe", C.c_void_p), ("h_packed", C.c_void_p), ("seed", C.c_uint32), ("byte_offset", C.c_uint64),
                ("h_out", C.c_void_p), ("out_capacity", C.c_size_t), ("n_out", C.c_size_t), ("ticket", C.c_int)]


class PddcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pddc error {code}: {msg}")
        self.code = code


def build(verbose: bool = False) -> None:
    """Compile csrc/ for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "all"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)


class StageDesc(C.Structure):
    _fields_ = [("decim", C.c_int), ("ntaps", C.c_int), ("taps", C.POINTER(C.c_float)),
                ("interp", C.c_int)]


class DemodRx(C.Structure):
    """pddc_demod_rx (include/perseus_ddc.h)"""
    _fields_ = [("mode", C.c_int), ("bfo", C.c_uint32), ("flags", C.c_uint32)]


class DemodParams(C.Structure):
    """pddc_demod_params (include/perseus_ddc.h)"""
    _fields_ = [("rho", C.c_float), ("lam", C.c_float), ("target", C.c_float), ("gmax", C.c_float)]


class CarrierParams(C.Structure):
    """pddc_carrier_params (include/perseus_ddc.h)"""
    _fields_ = [("vmax", C.c_float), ("gamma", C.c_float), ("lock_thr", C.c_float)]


class CarrierRx(C.Structure):
    """pddc_carrier_rx (include/perseus_ddc.h)"""
    _fields_ = [("mode", C.c_int), ("kp", C.c_float), ("ki", C.c_float)]


class SquelchParams(C.Structure):
    """pddc_squelch_params (include/perseus_ddc.h)"""
    _fields_ = [("block", C.c_int), ("attack", C.c_int), ("hang", C.c_int), ("ramp", C.c_int), ("up", C.c_float)]


class SquelchRx(C.Structure):
    """pddc_squelch_rx (include/perseus_ddc.h)"""
    _fields_ = [("open_thr", C.c_float), ("close_thr", C.c_float), ("flags", C.c_uint32)]


class AdaptParams(C.Structure):
    """pddc_adapt_params (include/perseus_ddc.h)"""
    _fields_ = [("taps", C.c_int), ("delay", C.c_int), ("eps", C.c_float)]


class AdaptRx(C.Structure):
    """pddc_adapt_rx (include/perseus_ddc.h)"""
    _fields_ = [("mode", C.c_uint32), ("mu", C.c_float), ("leak", C.c_float), ("flags", C.c_uint32)]


class DenoiseParams(C.Structure):
    """pddc_denoise_params (include/perseus_ddc.h)"""
    _fields_ = [("nfft", C.c_int), ("hop", C.c_int), ("smooth", C.c_float), ("up", C.c_float), ("down", C.c_float),
                ("nmin", C.c_float), ("eps", C.c_float)]


class DenoiseRx(C.Structure):
    """pddc_denoise_rx (include/perseus_ddc.h)"""
    _fields_ = [("mode", C.c_uint32), ("beta", C.c_float), ("gmin", C.c_float), ("alpha", C.c_float), ("flags", C.c_uint32)]


class EqSection(C.Structure):
    """pddc_eq_section (include/perseus_ddc.h): b0, b1, b2, a1, a2 with a0 = 1, binary64"""
    _fields_ = [("b0", C.c_double), ("b1", C.c_double), ("b2", C.c_double), ("a1", C.c_double), ("a2", C.c_double)]

    def __iter__(self):
        return iter((self.b0, self.b1, self.b2, self.a1, self.a2))


class EqParams(C.Structure):
    """pddc_eq_params (include/perseus_ddc.h)"""
    _fields_ = [("sections", C.c_int)]


class MixerParams(C.Structure):
    """pddc_mixer_params (include/perseus_ddc.h)"""
    _fields_ = [("nbus", C.c_int), ("ramp", C.c_int), ("flags", C.c_uint32), ("block", C.c_int), ("ceil", C.c_float),
                ("rel", C.c_float), ("scale", C.c_float)]


class FskRx(C.Structure):
    """pddc_fsk_rx"""
    _fields_ = [("modem", C.c_int), ("flags", C.c_uint32)]


class MorseRx(C.Structure):
    """pddc_morse_rx"""
    _fields_ = [("keyer", C.c_int), ("flags", C.c_uint32)]


class PskRx(C.Structure):
    """pddc_psk_rx"""
    _fields_ = [("modem", C.c_int), ("flags", C.c_uint32)]


class PskModem(C.Structure):
    """pddc_psk_modem"""
    _fields_ = [("inc", C.c_uint32), ("q", C.c_uint32), ("step", C.c_uint32)]


class SitorRx(C.Structure):
    """pddc_sitor_rx"""
    _fields_ = [("modem", C.c_int), ("flags", C.c_uint32)]


class SitorModem(C.Structure):
    """pddc_sitor_modem"""
    _fields_ = [("inc", C.c_uint32), ("step", C.c_uint32), ("lock", C.c_uint32), ("unlock", C.c_uint32)]


class FaxRx(C.Structure):
    """pddc_fax_rx"""
    _fields_ = [("modem", C.c_int), ("flags", C.c_uint32)]


class FaxModem(C.Structure):
    """pddc_fax_modem"""
    _fields_ = [("inc", C.c_uint32), ("width", C.c_uint32), ("box", C.c_uint32), ("scale", C.c_float), ("bias", C.c_float),
                ("start_lo", C.c_uint16), ("start_hi", C.c_uint16), ("stop_lo", C.c_uint16), ("stop_hi", C.c_uint16),
                ("need", C.c_uint32)]


class MfskRx(C.Structure):
    """pddc_mfsk_rx"""
    _fields_ = [("modem", C.c_int), ("flags", C.c_uint32)]


class MfskModem(C.Structure):
    """pddc_mfsk_modem"""
    _fields_ = [("ntones", C.c_uint32), ("inc", C.c_uint32), ("q", C.c_uint32), ("step", C.c_uint32)]


class MorseKeyer(C.Structure):
    """pddc_morse_keyer"""
    _fields_ = [("two0", C.c_uint32), ("two_min", C.c_uint32), ("two_max", C.c_uint32), ("shift", C.c_uint32)]


class MorseParams(C.Structure):
    """pddc_morse_params"""
    _fields_ = [("a_on", C.c_float), ("a_off", C.c_float), ("rel", C.c_float), ("relf", C.c_float), ("ratio", C.c_float)]


class BlankerParams(C.Structure):
    """pddc_blanker_params (include/perseus_ddc.h)"""
    _fields_ = [("block", C.c_int), ("guard", C.c_int), ("ramp", C.c_int), ("beta", C.c_float), ("cap", C.c_float)]


class BlankerRx(C.Structure):
    """pddc_blanker_rx (include/perseus_ddc.h)"""
    _fields_ = [("thr", C.c_float), ("flags", C.c_uint32)]


class WBlankParams(C.Structure):
    """pddc_wblank_params (include/perseus_ddc.h)"""
    _fields_ = [("block", C.c_int), ("history", C.c_int), ("guard", C.c_int), ("ramp_log2", C.c_int)]


_ddc = None


def ddc_lib() -> C.CDLL:
    """Load libperseus_ddc.so; raises if it has not been built."""
    global _ddc
    if _ddc is not None:
        return _ddc
    if not os.path.exists(DDC_LIB):
        raise FileNotFoundError(
            f"{DDC_LIB} is missing: run __graft_entry__.build() (there is no CPU fallback)")
    try:
        # torch bundles its own libamdhip64.so.7; load it first so that this
        # process holds ONE HIP runtime and torch streams/pointers are valid here
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(DDC_LIB)
    vp, sz = C.c_void_p, C.c_size_t
    L.pddc_version.restype = C.c_int
    L.pddc_last_error.restype = C.c_char_p
    L.pddc_device_count.restype = C.c_int
    L.pddc_nco_freg.argtypes = [C.c_double, C.c_double]
    L.pddc_nco_freg.restype = C.c_uint32
    L.pddc_unpack24_f32.argtypes = [vp, sz, vp, vp]
    L.pddc_unpack24_i32.argtypes = [vp, sz, vp, vp]
    L.pddc_pack24_f32.argtypes = [vp, sz, vp, vp]
    L.pddc_synth_lcg.argtypes = [vp, sz, C.c_uint32, C.c_uint64, vp]
    L.pddc_set_device.argtypes = [C.c_int]
    L.pddc_malloc.argtypes = [C.POINTER(vp), sz]
    L.pddc_free.argtypes = [vp]
    L.pddc_malloc_apart.argtypes = [C.POINTER(vp), sz, vp, sz, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pddc_malloc_apart.restype = C.c_int
    L.pddc_memcpy_h2d.argtypes = [vp, vp, sz, vp]
    L.pddc_memcpy_d2h.argtypes = [vp, vp, sz, vp]
    L.pddc_stream_sync.argtypes = [vp]
    L.pddc_pipeline_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(StageDesc), C.c_int, C.c_uint32]
    L.pddc_pipeline_destroy.argtypes = [vp]
    L.pddc_pipeline_reset.argtypes = [vp]
    L.pddc_pipeline_seek.argtypes = [vp, C.c_uint64]
    L.pddc_pipeline_set_freg.argtypes = [vp, C.c_uint32]
    L.pddc_pipeline_set_center_freq.argtypes = [vp, C.c_double]
    L.pddc_pipeline_set_taps.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int]
    L.pddc_pipeline_get_freg.argtypes = [vp]
    L.pddc_pipeline_get_freg.restype = C.c_uint32
    L.pddc_pipeline_get_phase_offset.argtypes = [vp]
    L.pddc_pipeline_get_phase_offset.restype = C.c_uint32
    L.pddc_pipeline_total_decim.argtypes = [vp]
    L.pddc_pipeline_max_output.argtypes = [vp, sz]
    L.pddc_pipeline_max_output.restype = sz
    L.pddc_pipeline_uses_fused.argtypes = [vp]
    L.pddc_pipeline_stage0_reads_packed.argtypes = [vp]
    L.pddc_pipeline_stage0_reads_packed.restype = C.c_int
    L.pddc_pipeline_uses_fused_pair.argtypes = [vp, sz]
    L.pddc_pipeline_uses_fused_pair.restype = C.c_int
    L.pddc_pipeline_uses_fused_cascade.argtypes = [vp, sz]
    L.pddc_pipeline_uses_fused_cascade.restype = C.c_int
    L.pddc_pipeline_stage0_on_i8.argtypes = [vp, sz]
    L.pddc_pipeline_stage0_on_i8.restype = C.c_int
    L.pddc_pipeline_arena_place.argtypes = [vp, vp, sz, sz, sz, sz, C.POINTER(sz), C.POINTER(C.c_float),
                                            C.POINTER(C.c_float), C.POINTER(C.c_int), vp]
    L.pddc_pipeline_arena_place.restype = C.c_int
    L.pddc_fir_i8_table.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, vp, sz, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pddc_fir_i8_table.restype = C.c_int
    L.pddc_fir_i8_taps16.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, vp, sz, C.POINTER(C.c_double)]
    L.pddc_fir_i8_taps16.restype = C.c_int
    L.pddc_fir_i8x_tables.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_uint32, vp, sz,
                                      C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pddc_fir_i8x_tables.restype = C.c_int
    L.pddc_fir_i8x_d10_tables.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_uint32, vp, sz,
                                          C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pddc_fir_i8x_d10_tables.restype = C.c_int
    L.pddc_fir_i8x_taps2.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_float), sz]
    L.pddc_fir_i8x_taps2.restype = C.c_int
    L.pddc_pipeline_set_option.argtypes = [vp, C.c_char_p, C.c_int]
    L.pddc_pipeline_set_option.restype = C.c_int
    L.pddc_pipeline_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
    L.pddc_pipeline_get_option.restype = C.c_int
    L.pddc_set_tunable.argtypes = [C.c_char_p, C.c_int]
    L.pddc_set_tunable.restype = C.c_int
    L.pddc_get_tunable.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    L.pddc_get_tunable.restype = C.c_int
    L.pddc_pipeline_check.argtypes = [vp, vp]
    L.pddc_pipeline_check.restype = C.c_int
    L.pddc_comm_rccl_version.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pddc_comm_rccl_version.restype = C.c_int
    L.pddc_pipeline_place_buffers.argtypes = [vp, vp, sz, vp]
    L.pddc_pipeline_place_buffers.restype = C.c_int
    L.pddc_pipeline_set_overlap.argtypes = [vp, C.c_int]
    L.pddc_pipeline_set_overlap.restype = C.c_int
    L.pddc_pipeline_fence.argtypes = [vp, vp]
    L.pddc_pipeline_fence.restype = C.c_int
    L.pddc_pipeline_process.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), vp]
    L.pddc_pipeline_push_host.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.pddc_pipeline_push_host_async.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(C.c_int)]
    L.pddc_pipeline_push_synth_async.argtypes = [vp, C.c_uint32, C.c_uint64, sz, vp, sz, C.POINTER(sz),
                                                 C.POINTER(C.c_int)]
    L.pddc_pipeline_push_synth_async.restype = C.c_int
    L.pddc_pipeline_ticket_done.argtypes = [vp, C.c_int]
    L.pddc_pipeline_ticket_done.restype = C.c_int
    L.pddc_pipeline_next_output.argtypes = [vp, sz]
    L.pddc_pipeline_next_output.restype = sz
    L.pddc_pipeline_wait_ticket.argtypes = [vp, C.c_int]
    L.pddc_pipeline_wait.argtypes = [vp]
    L.pddc_host_alloc.argtypes = [C.POINTER(vp), sz]
    L.pddc_host_free.argtypes = [vp]
    L.pddc_gang_create.argtypes = [C.POINTER(vp), C.c_int]
    L.pddc_gang_create.restype = C.c_int
    L.pddc_gang_destroy.argtypes = [vp]
    L.pddc_gang_destroy.restype = C.c_int
    L.pddc_gang_push_async.argtypes = [vp, C.POINTER(GangItem), C.c_int, sz, C.POINTER(C.c_int)]
    L.pddc_gang_push_async.restype = C.c_int
    L.pddc_bank_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int]
    L.pddc_bank_create.restype = C.c_int
    L.pddc_bank_destroy.argtypes = [vp]
    L.pddc_bank_destroy.restype = C.c_int
    L.pddc_bank_process.argtypes = [vp, vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_int), vp]
    L.pddc_bank_process.restype = C.c_int
    L.pddc_bank_schedule.argtypes = [vp, sz, C.POINTER(C.c_uint), C.POINTER(C.c_int)]
    L.pddc_bank_schedule.restype = C.c_int
    L.pddc_spectrum_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_uint32]
    L.pddc_spectrum_create.restype = C.c_int
    L.pddc_spectrum_destroy.argtypes = [vp]
    L.pddc_spectrum_reset.argtypes = [vp]
    L.pddc_spectrum_process.argtypes = [vp, vp, sz, vp]
    L.pddc_spectrum_read.argtypes = [vp, vp, vp, C.POINTER(C.c_uint64), C.c_int, vp]
    for f in (L.pddc_spectrum_destroy, L.pddc_spectrum_reset, L.pddc_spectrum_process, L.pddc_spectrum_read):
        f.restype = C.c_int
    L.pddc_spectrum_next_segments.argtypes = [vp, sz]
    L.pddc_spectrum_next_segments.restype = C.c_uint64
    L.pddc_spectrum_segments.argtypes = [C.c_int, C.c_int, C.c_uint64, sz]
    L.pddc_spectrum_segments.restype = C.c_uint64
    L.pddc_channelizer_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int,
                                          C.c_int, C.c_uint32]
    L.pddc_channelizer_destroy.argtypes = [vp]
    L.pddc_channelizer_reset.argtypes = [vp]
    L.pddc_channelizer_process.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), vp]
    L.pddc_channelizer_set_range.argtypes = [vp, C.c_int, C.c_int]
    L.pddc_channelizer_set_channels.argtypes = [vp, C.POINTER(C.c_int), C.c_int]
    for f in (L.pddc_channelizer_create, L.pddc_channelizer_destroy, L.pddc_channelizer_reset,
              L.pddc_channelizer_process, L.pddc_channelizer_set_range, L.pddc_channelizer_set_channels):
        f.restype = C.c_int
    L.pddc_channelizer_next_rows.argtypes = [vp, sz]
    L.pddc_channelizer_next_rows.restype = C.c_uint64
    L.pddc_channelizer_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, sz]
    L.pddc_channelizer_rows.restype = C.c_uint64
    L.pddc_tuner_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32),
                                    C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_uint32]
    L.pddc_tuner_destroy.argtypes = [vp]
    L.pddc_tuner_reset.argtypes = [vp]
    L.pddc_tuner_set_freq.argtypes = [vp, C.c_int, C.c_uint32]
    L.pddc_tuner_set_range.argtypes = [vp, C.c_int, C.c_int]
    L.pddc_tuner_process.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), vp]
    L.pddc_tuner_channel.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int32)]
    L.pddc_tuner_set_channels.argtypes = [vp, C.POINTER(C.c_int), C.c_int]
    L.pddc_tuner_channel_list.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int)]
    L.pddc_tuner_schedule.argtypes = [vp, sz, C.POINTER(C.c_int)]
    for f in (L.pddc_tuner_create, L.pddc_tuner_destroy, L.pddc_tuner_reset, L.pddc_tuner_set_freq,
              L.pddc_tuner_set_range, L.pddc_tuner_process, L.pddc_tuner_channel, L.pddc_tuner_set_channels,
              L.pddc_tuner_channel_list, L.pddc_tuner_schedule):
        f.restype = C.c_int
    L.pddc_tuner_next_outputs.argtypes = [vp, sz]
    L.pddc_tuner_next_outputs.restype = C.c_uint64
    L.pddc_tuner_outputs.argtypes = [C.c_int, C.c_int, C.c_uint64, sz]
    L.pddc_tuner_outputs.restype = C.c_uint64
    L.pddc_demod_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(DemodRx), C.POINTER(DemodParams)]
    L.pddc_demod_destroy.argtypes = [vp]
    L.pddc_demod_reset.argtypes = [vp]
    L.pddc_demod_set_rx.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32]
    L.pddc_demod_process.argtypes = [vp, vp, sz, sz, vp, sz, vp]
    L.pddc_demod_tile_outputs.argtypes = []
    for name in ("pddc_demod_create", "pddc_demod_destroy", "pddc_demod_reset", "pddc_demod_set_rx", "pddc_demod_process",
                 "pddc_demod_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_rxfilter_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.pddc_rxfilter_destroy.argtypes = [vp]
    L.pddc_rxfilter_reset.argtypes = [vp]
    L.pddc_rxfilter_set_rx.argtypes = [vp, C.c_int, C.c_int]
    L.pddc_rxfilter_process.argtypes = [vp, vp, sz, sz, vp, sz, vp]
    L.pddc_rxfilter_tile_outputs.argtypes = []
    for name in ("pddc_rxfilter_create", "pddc_rxfilter_destroy", "pddc_rxfilter_reset", "pddc_rxfilter_set_rx",
                 "pddc_rxfilter_process", "pddc_rxfilter_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_carrier_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(CarrierParams), C.POINTER(CarrierRx),
                                      C.POINTER(C.c_float), C.c_int]
    L.pddc_carrier_destroy.argtypes = [vp]
    L.pddc_carrier_reset.argtypes = [vp]
    L.pddc_carrier_set_rx.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_float]
    L.pddc_carrier_process.argtypes = [vp, vp, sz, sz, vp, sz, vp]
    L.pddc_carrier_read.argtypes = [vp, vp, vp]
    L.pddc_carrier_tile_outputs.argtypes = []
    L.pddc_carrier_group.argtypes = []
    for name in ("pddc_carrier_create", "pddc_carrier_destroy", "pddc_carrier_reset", "pddc_carrier_set_rx",
                 "pddc_carrier_process", "pddc_carrier_read", "pddc_carrier_tile_outputs", "pddc_carrier_group"):
        getattr(L, name).restype = C.c_int
    L.pddc_squelch_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(SquelchParams), C.POINTER(SquelchRx)]
    L.pddc_squelch_destroy.argtypes = [vp]
    L.pddc_squelch_reset.argtypes = [vp]
    L.pddc_squelch_set_rx.argtypes = [vp, C.c_int, C.c_float, C.c_float, C.c_uint32]
    L.pddc_squelch_process.argtypes = [vp, vp, vp, sz, sz, sz, vp, sz, vp, vp, sz, C.POINTER(sz), vp]
    L.pddc_squelch_next_blocks.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_squelch_read.argtypes = [vp, vp, C.c_int, vp]
    L.pddc_squelch_tile_outputs.argtypes = []
    for name in ("pddc_squelch_create", "pddc_squelch_destroy", "pddc_squelch_reset", "pddc_squelch_set_rx",
                 "pddc_squelch_process", "pddc_squelch_next_blocks", "pddc_squelch_read", "pddc_squelch_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_squelch_blocks.argtypes = [C.c_int, C.c_uint64, sz]
    L.pddc_squelch_blocks.restype = C.c_uint64
    L.pddc_adapt_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(AdaptParams), C.POINTER(AdaptRx)]
    L.pddc_adapt_destroy.argtypes = [vp]
    L.pddc_adapt_reset.argtypes = [vp]
    L.pddc_adapt_set_rx.argtypes = [vp, C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_uint32]
    L.pddc_adapt_process.argtypes = [vp, vp, sz, sz, vp, sz, vp]
    L.pddc_adapt_read_weights.argtypes = [vp, vp, vp]
    L.pddc_adapt_tile_outputs.argtypes = []
    for name in ("pddc_adapt_create", "pddc_adapt_destroy", "pddc_adapt_reset", "pddc_adapt_set_rx", "pddc_adapt_process",
                 "pddc_adapt_read_weights", "pddc_adapt_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_denoise_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(DenoiseParams), vp, C.POINTER(DenoiseRx)]
    L.pddc_denoise_destroy.argtypes = [vp]
    L.pddc_denoise_reset.argtypes = [vp]
    L.pddc_denoise_set_rx.argtypes = [vp, C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32]
    L.pddc_denoise_process.argtypes = [vp, vp, sz, sz, vp, sz, vp]
    L.pddc_denoise_read_noise.argtypes = [vp, vp, vp]
    L.pddc_denoise_delay.argtypes = [C.c_int]
    L.pddc_denoise_tile_frames.argtypes = []
    for name in ("pddc_denoise_create", "pddc_denoise_destroy", "pddc_denoise_reset", "pddc_denoise_set_rx",
                 "pddc_denoise_process", "pddc_denoise_read_noise", "pddc_denoise_delay", "pddc_denoise_tile_frames"):
        getattr(L, name).restype = C.c_int
    L.pddc_eq_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(EqParams), C.POINTER(C.c_int), C.POINTER(EqSection)]
    L.pddc_eq_destroy.argtypes = [vp]
    L.pddc_eq_reset.argtypes = [vp]
    L.pddc_eq_set_rx.argtypes = [vp, C.c_int, C.c_int, C.POINTER(EqSection), C.c_uint32]
    L.pddc_eq_process.argtypes = [vp, vp, sz, sz, vp, sz, vp]
    L.pddc_eq_read_state.argtypes = [vp, vp, vp]
    L.pddc_eq_tile_outputs.argtypes = []
    L.pddc_eq_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(EqSection)]
    for name in ("pddc_eq_create", "pddc_eq_destroy", "pddc_eq_reset", "pddc_eq_set_rx", "pddc_eq_process",
                 "pddc_eq_read_state", "pddc_eq_tile_outputs", "pddc_eq_design"):
        getattr(L, name).restype = C.c_int
    L.pddc_blanker_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(BlankerParams), C.POINTER(BlankerRx)]
    L.pddc_blanker_destroy.argtypes = [vp]
    L.pddc_blanker_reset.argtypes = [vp]
    L.pddc_blanker_set_rx.argtypes = [vp, C.c_int, C.c_float, C.c_uint32]
    L.pddc_blanker_process.argtypes = [vp, vp, sz, sz, vp, sz, vp]
    L.pddc_blanker_read.argtypes = [vp, vp, vp]
    L.pddc_blanker_delay.argtypes = [vp]
    L.pddc_blanker_tile_outputs.argtypes = []
    for name in ("pddc_blanker_create", "pddc_blanker_destroy", "pddc_blanker_reset", "pddc_blanker_set_rx",
                 "pddc_blanker_process", "pddc_blanker_read", "pddc_blanker_delay", "pddc_blanker_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_wblank_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(WBlankParams), C.c_uint32, C.c_uint32]
    L.pddc_wblank_destroy.argtypes = [vp]
    L.pddc_wblank_reset.argtypes = [vp]
    L.pddc_wblank_set.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.pddc_wblank_process.argtypes = [vp, vp, sz, vp, vp]
    L.pddc_wblank_read.argtypes = [vp, vp, vp]
    L.pddc_wblank_delay.argtypes = [vp]
    L.pddc_wblank_tile_samples.argtypes = []
    L.pddc_wblank_run_samples.argtypes = []
    for name in ("pddc_wblank_create", "pddc_wblank_destroy", "pddc_wblank_reset", "pddc_wblank_set", "pddc_wblank_process",
                 "pddc_wblank_read", "pddc_wblank_delay", "pddc_wblank_tile_samples", "pddc_wblank_run_samples"):
        getattr(L, name).restype = C.c_int
    L.pddc_scope_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                    C.POINTER(C.c_float), C.c_uint32]
    L.pddc_scope_destroy.argtypes = [vp]
    L.pddc_scope_reset.argtypes = [vp]
    L.pddc_scope_set_slot.argtypes = [vp, C.c_int, C.c_int]
    L.pddc_scope_process.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(sz), vp]
    L.pddc_scope_block_items.argtypes = [C.c_int]
    for name in ("pddc_scope_create", "pddc_scope_destroy", "pddc_scope_reset", "pddc_scope_set_slot", "pddc_scope_process",
                 "pddc_scope_block_items"):
        getattr(L, name).restype = C.c_int
    L.pddc_scope_next_lines.argtypes = [vp, sz]
    L.pddc_scope_next_lines.restype = C.c_uint64
    L.pddc_scope_lines.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, sz]
    L.pddc_scope_lines.restype = C.c_uint64
    L.pddc_audio_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                    C.POINTER(C.c_float), C.c_float]
    L.pddc_audio_destroy.argtypes = [vp]
    L.pddc_audio_reset.argtypes = [vp]
    L.pddc_audio_next_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_audio_process.argtypes = [vp, vp, sz, sz, vp, sz, vp, sz, C.POINTER(sz), vp]
    for name in ("pddc_audio_create", "pddc_audio_destroy", "pddc_audio_reset", "pddc_audio_next_outputs", "pddc_audio_process"):
        getattr(L, name).restype = C.c_int
    L.pddc_audio_outputs.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, sz]
    L.pddc_audio_outputs.restype = C.c_uint64
    L.pddc_mixer_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(MixerParams), C.POINTER(C.c_float)]
    L.pddc_mixer_destroy.argtypes = [vp]
    L.pddc_mixer_reset.argtypes = [vp]
    L.pddc_mixer_set_rx.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.pddc_mixer_next_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_mixer_process.argtypes = [vp, vp, sz, sz, vp, sz, vp, sz, C.POINTER(sz), vp]
    L.pddc_mixer_read.argtypes = [vp, vp, C.c_int, vp]
    L.pddc_mixer_chunk.argtypes = []
    L.pddc_mixer_tile_outputs.argtypes = []
    for name in ("pddc_mixer_create", "pddc_mixer_destroy", "pddc_mixer_reset", "pddc_mixer_set_rx", "pddc_mixer_next_outputs",
                 "pddc_mixer_process", "pddc_mixer_read", "pddc_mixer_chunk", "pddc_mixer_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_mixer_outputs.argtypes = [C.c_int, C.c_uint64, sz]
    L.pddc_mixer_outputs.restype = C.c_uint64
    L.pddc_fsk_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_int), C.POINTER(FskRx)]
    L.pddc_fsk_destroy.argtypes = [vp]
    L.pddc_fsk_reset.argtypes = [vp]
    L.pddc_fsk_set_rx.argtypes = [vp, C.c_int, C.c_int, C.c_uint32]
    L.pddc_fsk_max_chars.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_fsk_process.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp, sz, vp]
    L.pddc_fsk_read.argtypes = [vp, vp, vp]
    L.pddc_fsk_tile_outputs.argtypes = []
    for name in ("pddc_fsk_create", "pddc_fsk_destroy", "pddc_fsk_reset", "pddc_fsk_set_rx", "pddc_fsk_max_chars",
                 "pddc_fsk_process", "pddc_fsk_read", "pddc_fsk_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_morse_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(MorseKeyer),
                                    C.POINTER(MorseParams), C.POINTER(MorseRx)]
    L.pddc_morse_destroy.argtypes = [vp]
    L.pddc_morse_reset.argtypes = [vp]
    L.pddc_morse_set_rx.argtypes = [vp, C.c_int, C.c_int, C.c_uint32]
    L.pddc_morse_max_chars.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_morse_process.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp, sz, vp]
    L.pddc_morse_read.argtypes = [vp, vp, vp]
    L.pddc_morse_tile_outputs.argtypes = []
    for name in ("pddc_morse_create", "pddc_morse_destroy", "pddc_morse_reset", "pddc_morse_set_rx", "pddc_morse_max_chars",
                 "pddc_morse_process", "pddc_morse_read", "pddc_morse_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_psk_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(PskModem),
                                  C.POINTER(PskRx)]
    L.pddc_psk_destroy.argtypes = [vp]
    L.pddc_psk_reset.argtypes = [vp]
    L.pddc_psk_set_rx.argtypes = [vp, C.c_int, C.c_int, C.c_uint32]
    L.pddc_psk_max_syms.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_psk_max_chars.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_psk_process.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, vp]
    L.pddc_psk_read.argtypes = [vp, vp, vp]
    L.pddc_psk_tile_outputs.argtypes = []
    for name in ("pddc_psk_create", "pddc_psk_destroy", "pddc_psk_reset", "pddc_psk_set_rx", "pddc_psk_max_syms", "pddc_psk_max_chars",
                 "pddc_psk_process", "pddc_psk_read", "pddc_psk_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_sitor_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(SitorModem),
                                    C.POINTER(SitorRx)]
    L.pddc_sitor_destroy.argtypes = [vp]
    L.pddc_sitor_reset.argtypes = [vp]
    L.pddc_sitor_set_rx.argtypes = [vp, C.c_int, C.c_int, C.c_uint32]
    L.pddc_sitor_max_syms.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_sitor_max_chars.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_sitor_process.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, vp]
    L.pddc_sitor_read.argtypes = [vp, vp, vp]
    L.pddc_sitor_tile_outputs.argtypes = []
    for name in ("pddc_sitor_create", "pddc_sitor_destroy", "pddc_sitor_reset", "pddc_sitor_set_rx", "pddc_sitor_max_syms",
                 "pddc_sitor_max_chars", "pddc_sitor_process", "pddc_sitor_read", "pddc_sitor_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_fax_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(FaxModem),
                                  C.POINTER(FaxRx)]
    L.pddc_fax_destroy.argtypes = [vp]
    L.pddc_fax_reset.argtypes = [vp]
    L.pddc_fax_set_rx.argtypes = [vp, C.c_int, C.c_int, C.c_uint32]
    L.pddc_fax_max_pixels.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_fax_max_lines.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_fax_process.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, vp, sz, vp]
    L.pddc_fax_read.argtypes = [vp, vp, vp]
    L.pddc_fax_tile_outputs.argtypes = []
    for name in ("pddc_fax_create", "pddc_fax_destroy", "pddc_fax_reset", "pddc_fax_set_rx", "pddc_fax_max_pixels", "pddc_fax_max_lines",
                 "pddc_fax_process", "pddc_fax_read", "pddc_fax_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_mfsk_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(MfskModem),
                                   C.POINTER(MfskRx)]
    L.pddc_mfsk_destroy.argtypes = [vp]
    L.pddc_mfsk_reset.argtypes = [vp]
    L.pddc_mfsk_set_rx.argtypes = [vp, C.c_int, C.c_int, C.c_uint32]
    L.pddc_mfsk_max_syms.argtypes = [vp, sz, C.POINTER(sz)]
    L.pddc_mfsk_process.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp, sz, vp]
    L.pddc_mfsk_read.argtypes = [vp, vp, vp]
    L.pddc_mfsk_tile_outputs.argtypes = []
    for name in ("pddc_mfsk_create", "pddc_mfsk_destroy", "pddc_mfsk_reset", "pddc_mfsk_set_rx", "pddc_mfsk_max_syms", "pddc_mfsk_process",
                 "pddc_mfsk_read", "pddc_mfsk_tile_outputs"):
        getattr(L, name).restype = C.c_int
    L.pddc_pipeline_time_stage0.argtypes = [vp, vp, sz, vp, C.c_int, vp, C.POINTER(C.c_float)]
    L.pddc_pipeline_time_stage0_inline.argtypes = [vp, C.c_int]
    L.pddc_pipeline_time_stage0_inline.restype = C.c_int
    L.pddc_pipeline_stage0_time.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.pddc_pipeline_stage0_time.restype = C.c_int
    L.pddc_pipeline_state_size.argtypes = [vp]
    L.pddc_pipeline_state_size.restype = sz
    L.pddc_pipeline_save_state.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.pddc_pipeline_save_state.restype = C.c_int
    L.pddc_pipeline_restore_state.argtypes = [vp, vp, sz]
    L.pddc_pipeline_restore_state.restype = C.c_int
    L.pddc_pipeline_workspace_size.argtypes = [vp, sz]
    L.pddc_pipeline_workspace_size.restype = sz
    L.pddc_pipeline_set_workspace.argtypes = [vp, vp, sz, sz]
    L.pddc_pipeline_set_workspace.restype = C.c_int
    L.pddc_pipeline_inject_failure.argtypes = [vp, C.c_int]
    L.pddc_pipeline_inject_failure.restype = C.c_int
    L.pddc_pipeline_schedule.argtypes = [vp, sz, C.POINTER(C.c_int)]
    L.pddc_pipeline_schedule.restype = C.c_int
    L.pddc_measure_copy.argtypes = [vp, vp, sz, C.c_int, vp, C.POINTER(C.c_float)]
    L.pddc_measure_copy.restype = C.c_int
    # multi-GPU section (RCCL, ddc_multi.cpp)
    L.pddc_comm_get_unique_id.argtypes = [vp]
    L.pddc_comm_init_rank.argtypes = [C.POINTER(vp), C.c_int, C.c_int, vp, C.c_int]
    L.pddc_comm_init_all.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int)]
    L.pddc_comm_destroy.argtypes = [vp]
    L.pddc_comm_rank.argtypes = [vp]
    L.pddc_comm_size.argtypes = [vp]
    L.pddc_comm_device.argtypes = [vp]
    L.pddc_comm_bcast.argtypes = [vp, vp, sz, C.c_int, vp]
    L.pddc_comm_bcast_host.argtypes = [vp, vp, sz, C.c_int]
    L.pddc_comm_allreduce_max_f64.argtypes = [vp, C.POINTER(C.c_double)]
    L.pddc_comm_barrier.argtypes = [vp]
    L.pddc_comm_gather.argtypes = [vp, vp, sz, vp, C.c_int, vp]
    L.pddc_comm_gather_async.argtypes = [vp, vp, sz, vp, C.c_int, vp]
    L.pddc_comm_gather_fence.argtypes = [vp, vp]
    L.pddc_comm_gather_wait.argtypes = [vp]
    L.pddc_plan_pack.argtypes = [C.POINTER(StageDesc), C.c_int, C.c_uint32, C.c_uint32, vp, sz]
    L.pddc_plan_pack.restype = sz
    L.pddc_plan_unpack.argtypes = [vp, sz, C.POINTER(StageDesc), C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint32)]
    L.pddc_comm_bcast_pipeline.argtypes = [vp, C.c_int, C.POINTER(StageDesc), C.c_int, C.c_uint32, C.c_uint32,
                                           C.POINTER(vp)]
    for name in ("pddc_comm_get_unique_id", "pddc_comm_init_rank", "pddc_comm_init_all", "pddc_comm_destroy",
                 "pddc_comm_rank", "pddc_comm_size", "pddc_comm_device", "pddc_comm_group_start",
                 "pddc_comm_group_end", "pddc_comm_bcast", "pddc_comm_bcast_host", "pddc_comm_allreduce_max_f64",
                 "pddc_comm_barrier", "pddc_comm_gather", "pddc_comm_gather_async", "pddc_comm_gather_fence",
                 "pddc_comm_gather_wait", "pddc_plan_unpack", "pddc_comm_bcast_pipeline"):
        getattr(L, name).restype = C.c_int
    for name in ("pddc_unpack24_f32", "pddc_unpack24_i32", "pddc_pack24_f32", "pddc_synth_lcg", "pddc_set_device",
                 "pddc_malloc", "pddc_free", "pddc_memcpy_h2d", "pddc_memcpy_d2h", "pddc_stream_sync",
                 "pddc_pipeline_create", "pddc_pipeline_destroy", "pddc_pipeline_reset", "pddc_pipeline_seek",
                 "pddc_pipeline_set_freg", "pddc_pipeline_set_center_freq", "pddc_pipeline_set_taps",
                 "pddc_pipeline_total_decim", "pddc_pipeline_uses_fused", "pddc_pipeline_process",
                 "pddc_pipeline_push_host", "pddc_pipeline_time_stage0", "pddc_pipeline_push_host_async",
                 "pddc_pipeline_wait_ticket", "pddc_pipeline_wait", "pddc_host_alloc", "pddc_host_free"):
        getattr(L, name).restype = C.c_int
    _ddc = L
    return L


def set_tunable(name: str, value: int):
    """process-wide development knob of the launchers (pddc_set_tunable)"""
    check(ddc_lib().pddc_set_tunable(name.encode(), int(value)))


def get_tunable(name: str) -> int:
    v = C.c_int(0)
    check(ddc_lib().pddc_get_tunable(name.encode(), C.byref(v)))
    return int(v.value)


def check(rc: int) -> int:
    if rc < 0:
        raise PddcError(rc, ddc_lib().pddc_last_error().decode(errors="replace"))
    return rc


class Pipeline:
    """Thin handle over pddc_pipeline_* (include/perseus_ddc.h)."""

    def __init__(self, stages, device: int = 0, mix: bool = False, taps_fp16: bool = False,
                 no_fast: bool = False, out_packed: bool = False):
        import numpy as np
        L = ddc_lib()
        self._taps = [np.ascontiguousarray(st[1], dtype=np.float32) for st in stages]
        arr = (StageDesc * len(stages))()
        for i, st in enumerate(stages):
            arr[i].decim = int(st[0])
            arr[i].interp = int(st[2]) if len(st) > 2 and st[2] else 0
            arr[i].ntaps = int(self._taps[i].size)
            arr[i].taps = self._taps[i].ctypes.data_as(C.POINTER(C.c_float))
        flags = (PDDC_F_MIX if mix else 0) | (PDDC_F_TAPS_FP16 if taps_fp16 else 0) | \
                (PDDC_F_NO_FAST if no_fast else 0) | (PDDC_F_OUT_PACKED24 if out_packed else 0)
        self.out_packed = out_packed
        h = C.c_void_p()
        check(L.pddc_pipeline_create(C.byref(h), device, arr, len(stages), flags))
        self._h = h
        self.decim = L.pddc_pipeline_total_decim(h)

    @classmethod
    def from_handle(cls, handle, out_packed: bool = False):
        """Wrap a pddc_pipeline* made by the library itself (Comm.bcast_pipeline)."""
        self = cls.__new__(cls)
        self._taps = []
        self.out_packed = out_packed
        self._h = handle
        self.decim = ddc_lib().pddc_pipeline_total_decim(handle)
        return self

    def close(self):
        if getattr(self, "_h", None):
            ddc_lib().pddc_pipeline_destroy(self._h)
            self._h = None

    __del__ = close

    def reset(self):
        check(ddc_lib().pddc_pipeline_reset(self._h))

    def seek(self, abs_sample: int):
        """Zero history, stream positioned at absolute input sample `abs_sample` (NCO and
        decimation phases of a stream that started at 0): time-chunk sharding, shard.py."""
        check(ddc_lib().pddc_pipeline_seek(self._h, int(abs_sample)))

    def set_freg(self, freg: int):
        check(ddc_lib().pddc_pipeline_set_freg(self._h, freg & 0xFFFFFFFF))

    def set_center_freq(self, hz: float):
        check(ddc_lib().pddc_pipeline_set_center_freq(self._h, float(hz)))

    @property
    def freg(self) -> int:
        return int(ddc_lib().pddc_pipeline_get_freg(self._h))

    @property
    def phase_offset(self) -> int:
        """phase(n) = n*freg + phase_offset (mod 2^32); non-zero only after a retune mid-stream."""
        return int(ddc_lib().pddc_pipeline_get_phase_offset(self._h))

    @property
    def fused(self) -> bool:
        return bool(ddc_lib().pddc_pipeline_uses_fused(self._h))

    @property
    def stage0_reads_packed(self) -> bool:
        return bool(ddc_lib().pddc_pipeline_stage0_reads_packed(self._h))

    def fused_pair(self, nsamples: int) -> int:
        """0: stages 0 and 1 are separate kernels; 1: k_fir8's fused pair; 2: k_fir_i8x's (matrix cores, NCO in the taps)"""
        return int(ddc_lib().pddc_pipeline_uses_fused_pair(self._h, nsamples))

    def set_option(self, name: str, value: int):
        """kernel selection as API state: no_i8, i8x, i8x_pair, i8x_plain, i8x_blocks, no_fuse2, fuse3"""
        check(ddc_lib().pddc_pipeline_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int(0)
        check(ddc_lib().pddc_pipeline_get_option(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def fused_cascade(self, nsamples: int) -> bool:
        """stages 0, 1 and 2 as one kernel for a batch of this size"""
        return bool(ddc_lib().pddc_pipeline_uses_fused_cascade(self._h, nsamples))

    def on_i8(self, nsamples: int) -> int:
        """stage 0 of a batch of nsamples runs on the int8 matrix cores: 0 no (k_fir8), 2 k_fir_i8x (plain, or the NCO folded
        into the taps; 1 was round 3's k_fir_i8, retired)"""
        return int(ddc_lib().pddc_pipeline_stage0_on_i8(self._h, nsamples))

    def check(self, stream: int = 0):
        """wait for `stream`; raises if a kernel of this pipeline flagged a failure"""
        check(ddc_lib().pddc_pipeline_check(self._h, stream))

    def place_buffers(self, d_in: int, max_nsamples: int, stream: int = 0):
        """allocate the pipeline's own inter-stage buffers away (in HBM extent class) from the batch they are made from"""
        check(ddc_lib().pddc_pipeline_place_buffers(self._h, d_in, max_nsamples, stream))

    def set_overlap(self, enable: bool = True):
        """the last stage (behind k_fir8's fused pair or first stage) is held back and rides along with the NEXT batch's
        first-stage launch as extra thread blocks; fence() launches what is still held back (see perseus_ddc.h)"""
        check(ddc_lib().pddc_pipeline_set_overlap(self._h, 1 if enable else 0))

    def fence(self, stream: int = 0):
        """launches the tail overlap mode still holds back on `stream` (call before reading the last output)"""
        check(ddc_lib().pddc_pipeline_fence(self._h, stream))

    def max_output(self, n: int) -> int:
        return int(ddc_lib().pddc_pipeline_max_output(self._h, n))

    def process_ptr(self, d_in: int, nsamples: int, d_out: int, out_cap: int, stream: int = 0) -> int:
        n = C.c_size_t(0)
        check(ddc_lib().pddc_pipeline_process(self._h, d_in, nsamples, d_out, out_cap, C.byref(n), stream))
        return n.value

    def process(self, packed_u8, out_f32=None, stream=None):
        """packed_u8: torch uint8 CUDA tensor; returns torch float32 tensor [n_out, 2]."""
        import torch
        ns = packed_u8.numel() // 6
        cap = self.max_output(ns) + 1
        st = stream if stream is not None else torch.cuda.current_stream(packed_u8.device).cuda_stream
        if self.out_packed:                       # 6 bytes per output sample
            out_u8 = torch.empty(6 * cap + 16, dtype=torch.uint8, device=packed_u8.device)
            n = self.process_ptr(packed_u8.data_ptr(), ns, out_u8.data_ptr(), cap, st)
            self.fence(st)
            return out_u8[:6 * n]
        if out_f32 is None:
            out_f32 = torch.empty((cap, 2), dtype=torch.float32, device=packed_u8.device)
        n = self.process_ptr(packed_u8.data_ptr(), ns, out_f32.data_ptr(), out_f32.numel() // 2, st)
        self.fence(st)                            # overlap mode: the caller is about to read this output
        return out_f32[:n]

    def push_host(self, packed_np):
        import numpy as np
        b = np.ascontiguousarray(packed_np, dtype=np.uint8)
        ns = b.size // 6
        cap = self.max_output(ns) + 1
        out = np.empty((cap, 2), dtype=np.float32)
        n = C.c_size_t(0)
        check(ddc_lib().pddc_pipeline_push_host(self._h, b.ctypes.data, ns, out.ctypes.data, cap, C.byref(n)))
        return out[:n.value]

    def push_host_async(self, h_in: int, nsamples: int, h_out: int, out_cap: int):
        """Raw-pointer form (pinned buffers from host_alloc): returns (n_out, ticket)."""
        n, t = C.c_size_t(0), C.c_int(-1)
        check(ddc_lib().pddc_pipeline_push_host_async(self._h, h_in, nsamples, h_out, out_cap, C.byref(n), C.byref(t)))
        return n.value, t.value

    def push_synth_async(self, seed: int, byte_offset: int, nsamples: int, h_out: int, out_cap: int):
        """Device-generated LCG batch (no H2D): returns (n_out, ticket)."""
        n, t = C.c_size_t(0), C.c_int(-1)
        check(ddc_lib().pddc_pipeline_push_synth_async(self._h, seed & 0xFFFFFFFF, byte_offset, nsamples, h_out,
                                                       out_cap, C.byref(n), C.byref(t)))
        return n.value, t.value

    def next_output(self, n: int) -> int:
        return int(ddc_lib().pddc_pipeline_next_output(self._h, n))

    def wait_ticket(self, ticket: int):
        check(ddc_lib().pddc_pipeline_wait_ticket(self._h, ticket))

    def wait(self):
        check(ddc_lib().pddc_pipeline_wait(self._h))

    def workspace_size(self, max_nsamples: int) -> int:
        """Bytes of caller-provided device memory the inter-stage buffers need for batches up to max_nsamples."""
        return int(ddc_lib().pddc_pipeline_workspace_size(self._h, max_nsamples))

    def set_workspace(self, d_ws: int | None, nbytes: int = 0, max_nsamples: int = 0):
        """Inter-stage buffers from the caller's memory (pddc_pipeline_set_workspace); None: own allocations again."""
        check(ddc_lib().pddc_pipeline_set_workspace(self._h, d_ws, nbytes, max_nsamples))

    def save_state(self) -> bytes:
        """The stream state as one blob (histories, decimation phases, sample counter, NCO)."""
        L = ddc_lib()
        n = L.pddc_pipeline_state_size(self._h)
        buf = C.create_string_buffer(n)
        used = C.c_size_t(0)
        check(L.pddc_pipeline_save_state(self._h, buf, n, C.byref(used)))
        return buf.raw[:used.value]

    def restore_state(self, blob: bytes):
        check(ddc_lib().pddc_pipeline_restore_state(self._h, C.create_string_buffer(blob, len(blob)), len(blob)))

    def schedule(self, nsamples: int) -> dict:
        """Tile schedule of the fused stage-0 kernel for a batch of nsamples."""
        o = (C.c_int * 5)()
        check(ddc_lib().pddc_pipeline_schedule(self._h, nsamples, o))
        return {"tile": o[0], "ntiles": o[1], "nblocks": o[2], "S": o[3], "K": o[4]}

    def time_stage0_inline(self, enable: bool):
        """Bracket the stage-0 kernel of every process() with HIP events (read with stage0_time)."""
        check(ddc_lib().pddc_pipeline_time_stage0_inline(self._h, 1 if enable else 0))

    def stage0_time(self):
        """-> (average ms of the stage-0 kernel over the process() calls since enabled, number of calls)."""
        ms, n = C.c_float(0), C.c_int(0)
        check(ddc_lib().pddc_pipeline_stage0_time(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def time_stage0(self, d_in: int, nsamples: int, d_out: int, iters: int, stream: int = 0) -> float:
        ms = C.c_float(0)
        check(ddc_lib().pddc_pipeline_time_stage0(self._h, d_in, nsamples, d_out, iters, stream, C.byref(ms)))
        return float(ms.value)


def _stage_array(stages):
    """[(D, taps[, L])] -> (StageDesc array, the numpy arrays that own the taps)."""
    import numpy as np
    keep = [np.ascontiguousarray(st[1], dtype=np.float32) for st in stages]
    arr = (StageDesc * max(len(stages), 1))()
    for i, st in enumerate(stages):
        arr[i].decim = int(st[0])
        arr[i].interp = int(st[2]) if len(st) > 2 and st[2] else 0
        arr[i].ntaps = int(keep[i].size)
        arr[i].taps = keep[i].ctypes.data_as(C.POINTER(C.c_float))
    return arr, keep


def plan_pack(stages, freg: int = 0, flags: int = 0) -> bytes:
    """pddc_plan_pack: the flat buffer a configuration broadcast carries."""
    L = ddc_lib()
    arr, _keep = _stage_array(stages)
    need = L.pddc_plan_pack(arr, len(stages), freg & 0xFFFFFFFF, flags, None, 0)
    if need == 0:
        raise PddcError(PDDC_EINVAL, L.pddc_last_error().decode(errors="replace"))
    buf = C.create_string_buffer(need)
    used = L.pddc_plan_pack(arr, len(stages), freg & 0xFFFFFFFF, flags, buf, need)
    assert used == need
    return buf.raw


def plan_unpack(raw: bytes):
    """pddc_plan_unpack -> {"freg", "flags", "stages": [(D, taps, L)]}."""
    import numpy as np
    L = ddc_lib()
    buf = C.create_string_buffer(raw, len(raw))
    arr = (StageDesc * 4)()
    n, freg, flags = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
    check(L.pddc_plan_unpack(buf, len(raw), arr, C.byref(n), C.byref(freg), C.byref(flags)))
    stages = []
    for i in range(n.value):
        t = np.ctypeslib.as_array(arr[i].taps, shape=(arr[i].ntaps,)).copy()
        stages.append((arr[i].decim, t, arr[i].interp))
    return {"freg": freg.value, "flags": flags.value, "stages": stages}


class Comm:
    """One RCCL communicator rank on one GPU (pddc_comm_*, include/perseus_ddc.h): the
    C library calls librccl itself, torch is not involved."""

    def __init__(self, handle):
        self._h = handle
        L = ddc_lib()
        self.rank, self.size, self.device = L.pddc_comm_rank(handle), L.pddc_comm_size(handle), \
            L.pddc_comm_device(handle)

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(PDDC_COMM_ID_BYTES)
        check(ddc_lib().pddc_comm_get_unique_id(buf))
        return buf.raw

    @classmethod
    def init_rank(cls, nranks: int, rank: int, uid: bytes, device: int):
        h = C.c_void_p()
        check(ddc_lib().pddc_comm_init_rank(C.byref(h), nranks, rank, C.create_string_buffer(uid, len(uid)), device))
        return cls(h)

    @classmethod
    def init_all(cls, devices):
        n = len(devices)
        hs = (C.c_void_p * n)()
        check(ddc_lib().pddc_comm_init_all(hs, n, (C.c_int * n)(*devices)))
        return [cls(C.c_void_p(hs[i])) for i in range(n)]

    def close(self):
        if getattr(self, "_h", None):
            ddc_lib().pddc_comm_destroy(self._h)
            self._h = None

    def bcast(self, d_ptr: int, nbytes: int, root: int = 0, stream: int = 0):
        check(ddc_lib().pddc_comm_bcast(self._h, d_ptr, nbytes, root, stream))

    def bcast_bytes(self, raw, root: int = 0) -> bytes:
        """Host-level broadcast of a byte string whose length every rank knows."""
        buf = C.create_string_buffer(raw, len(raw))
        check(ddc_lib().pddc_comm_bcast_host(self._h, buf, len(raw), root))
        return buf.raw

    def bcast_pipeline(self, stages=None, freg: int = 0, flags: int = 0, root: int = 0) -> "Pipeline":
        """Root passes the plan; every rank returns a Pipeline built from the broadcast."""
        L = ddc_lib()
        h = C.c_void_p()
        if self.rank == root:
            arr, _keep = _stage_array(stages)
            check(L.pddc_comm_bcast_pipeline(self._h, root, arr, len(stages), freg & 0xFFFFFFFF, flags, C.byref(h)))
        else:
            check(L.pddc_comm_bcast_pipeline(self._h, root, None, 0, 0, 0, C.byref(h)))
        return Pipeline.from_handle(h, out_packed=bool(flags & PDDC_F_OUT_PACKED24))

    def max_f64(self, v: float) -> float:
        x = C.c_double(v)
        check(ddc_lib().pddc_comm_allreduce_max_f64(self._h, C.byref(x)))
        return x.value

    def barrier(self):
        check(ddc_lib().pddc_comm_barrier(self._h))

    def gather(self, d_send: int, nbytes: int, d_recv: int, root: int = 0, stream: int = 0):
        check(ddc_lib().pddc_comm_gather(self._h, d_send, nbytes, d_recv, root, stream))

    def gather_async(self, d_send: int, nbytes: int, d_recv: int, root: int = 0, after_stream: int = 0):
        check(ddc_lib().pddc_comm_gather_async(self._h, d_send, nbytes, d_recv, root, after_stream))

    def gather_fence(self, stream: int = 0):
        check(ddc_lib().pddc_comm_gather_fence(self._h, stream))

    def gather_wait(self):
        check(ddc_lib().pddc_comm_gather_wait(self._h))


class Gang:
    """pddc_gang: the pipelines of one GPU that stream together share one launch chain (include/perseus_ddc.h;
    the reference's eight descriptors behind one poll thread, perseus-sdr.c:43-47, 736-774)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check(ddc_lib().pddc_gang_create(C.byref(h), device))
        self._h = h

    def push_async(self, items, nsamples: int):
        """items: dicts with pipe (Pipeline), h_out (pinned pointer), out_cap and either h_packed (pinned pointer) or
        seed + byte_offset (on-device source).  -> ([(n_out, ticket)], number of members that shared launches)."""
        arr = (GangItem * len(items))()
        for a, it in zip(arr, items):
            a.pipe = it["pipe"]._h
            a.h_packed = it.get("h_packed")
            a.seed = it.get("seed", 0) & 0xFFFFFFFF
            a.byte_offset = it.get("byte_offset", 0)
            a.h_out = it["h_out"]
            a.out_capacity = it["out_cap"]
        ng = C.c_int()
        check(ddc_lib().pddc_gang_push_async(self._h, arr, len(items), nsamples, C.byref(ng)))
        return [(a.n_out, a.ticket) for a in arr], ng.value

    def close(self):
        if getattr(self, "_h", None):
            ddc_lib().pddc_gang_destroy(self._h)
            self._h = None

    __del__ = close


class Bank:
    """pddc_bank: up to PDDC_BANK_MAX pipelines of one GPU fed the same batch every round; the tuned first stages of up to
    four of them come from one read of it (include/perseus_ddc.h).  Decimate-by-8 members (<= 64 taps) are grouped by
    history length; decimate-by-10 members (the 1 / 1.6 / 2 MS/s plans) go in pairs of the same decimation phase, and one
    without a partner runs alone.  Destroy it before its pipelines."""

    def __init__(self, pipes, device: int = 0):
        self.pipes = list(pipes)                  # (keeps the members alive as long as the bank)
        arr = (C.c_void_p * len(self.pipes))(*[p._h.value if isinstance(p._h, C.c_void_p) else p._h for p in self.pipes])
        h = C.c_void_p()
        check(ddc_lib().pddc_bank_create(C.byref(h), device, arr, len(self.pipes)))
        self._h = h

    def process_ptr(self, d_in: int, nsamples: int, d_outs, caps, stream: int = 0):
        """One round: nsamples packed samples at device address d_in through every member; member i writes d_outs[i]
        (capacity caps[i] outputs).  -> (list of n_out, number of members whose first stage shared a bank launch)."""
        k = len(self.pipes)
        outs = (C.c_void_p * k)(*[int(d) for d in d_outs])
        cap = (C.c_size_t * k)(*[int(c) for c in caps])
        n = (C.c_size_t * k)()
        nb = C.c_int()
        check(ddc_lib().pddc_bank_process(self._h, d_in, nsamples, outs, cap, n, C.byref(nb), stream))
        return [int(v) for v in n], nb.value

    def schedule(self, nsamples: int):
        """-> (mask: bit i = member i shares a bank launch in the next round of nsamples, bank launches)"""
        mask, launches = C.c_uint(), C.c_int()
        check(ddc_lib().pddc_bank_schedule(self._h, nsamples, C.byref(mask), C.byref(launches)))
        return mask.value, launches.value

    def close(self):
        if getattr(self, "_h", None):
            ddc_lib().pddc_bank_destroy(self._h)
            self._h = None

    __del__ = close


PDDC_SPEC_PEAK = 0x1


def hann_window(nfft: int):
    """The periodic Hann window, float32[nfft]: 0.5 - 0.5 cos(2 pi n / nfft) in double, rounded once."""
    import numpy as np
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)).astype(np.float32)


def spectrum_dbfs(sum_, nsegments: int, window):
    """10 log10(P / (nsegments (sum w)^2)): a full-scale complex tone on a bin centre reads 0 dBFS.  `sum_` a torch tensor
    or an array (what Spectrum.read returns first), `window` the window the spectrum was made with.  -> numpy float64."""
    import numpy as np
    p = sum_.detach().cpu().numpy() if hasattr(sum_, "detach") else np.asarray(sum_)
    w = np.asarray(window, dtype=np.float64)
    ref = float(nsegments) * w.sum() ** 2
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(p.astype(np.float64) / ref)


def _channel_list(channels):
    """a channel list as the C ABI takes it -> (numpy int32 array, its int pointer)"""
    import numpy as np
    ch = np.ascontiguousarray(np.asarray(channels, dtype=np.int64).reshape(-1), dtype=np.int32)
    return ch, ch.ctypes.data_as(C.POINTER(C.c_int))


def _packed_arg(kind, packed, nsamples):
    """a torch uint8 CUDA tensor of packed samples, or a device address with nsamples -> (address, nsamples)"""
    if hasattr(packed, "data_ptr"):
        return packed.data_ptr(), packed.numel() // 6 if nsamples is None else nsamples
    if nsamples is None:
        raise PddcError(-1, f"{kind}: a device address needs nsamples")
    return int(packed), nsamples


def _clip(v) -> int:
    """an integer parameter as a C int: out of range stays out of range"""
    return max(-1, min(int(v), 1 << 30))


class _StreamObject:
    """What WBlank, Spectrum, Channelizer, Tuner, Blanker, RxFilter, Carrier, Scope, Demod, Squelch, Adapt, Denoise, Eq, Audio, Mixer, Fsk, Morse, Psk, Sitor, Fax and Mfsk share: `_h`, the handle of a pddc_<_kind>_* object on `device`."""
    _kind = ""

    def _stream(self, stream):
        import torch
        return stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream

    def _rows(self, t, dtype) -> bool:
        """t is what the per-receiver stages read and write: a `dtype` tensor [nrx, any] whose rows are contiguous"""
        return t.dtype == dtype and t.dim() == 2 and t.shape[0] == self.nrx and (t.shape[1] <= 1 or t.stride(1) == 1)

    def _out(self, out, count: int, dtype, what: str):
        """An output of `count` items per receiver: `out` if given (refused as "<kind>: <what> tensor [nrx, capacity] ..."
        unless it is such rows), a new tensor otherwise.  -> (out, the capacity for the C ABI).  The ABI takes row
        strides; a capacity below `count` must reach it as one (PDDC_ECAPACITY) whatever the view's stride."""
        if out is None:
            import torch
            out = torch.empty((self.nrx, count), dtype=dtype, device=torch.device("cuda", self.device))
        elif not self._rows(out, dtype):
            raise PddcError(-1, f"{self._kind}: {what} tensor [nrx, capacity] with contiguous rows")
        return out, int(out.stride(0)) if out.shape[1] >= count else int(out.shape[1])

    def reset(self):
        check(getattr(ddc_lib(), f"pddc_{self._kind}_reset")(self._h))

    def close(self):
        if getattr(self, "_h", None):
            getattr(ddc_lib(), f"pddc_{self._kind}_destroy")(self._h)
            self._h = None

    __del__ = close


class Spectrum(_StreamObject):
    """pddc_spectrum: the panorama -- |FFT|^2 of windowed segments of the packed ADC-rate stream, summed (and optionally
    peak-held) over the complete segments since the last clear (include/perseus_ddc.h).  nfft in 1024 / 2048 / 4096 / 8192,
    hop nfft (default) or nfft/2, window float32[nfft] (default: periodic Hann).  The segment grid belongs to the stream:
    batches may be cut anywhere on a multiple of 8 samples."""
    _kind = "spectrum"

    def __init__(self, nfft: int, hop=None, window=None, device: int = 0, peak: bool = False):
        import numpy as np
        self.nfft, self.hop, self.device, self.peak = int(nfft), int(nfft if hop is None else hop), device, bool(peak)
        if window is None:
            if self.nfft <= 0:
                raise PddcError(-1, "spectrum: nfft must be positive")
            window = hann_window(self.nfft)
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float32).reshape(-1))
        if w.size != self.nfft:
            raise PddcError(-1, f"spectrum: window of {w.size} values for nfft {self.nfft}")
        self.window = w
        h = C.c_void_p()
        check(ddc_lib().pddc_spectrum_create(C.byref(h), device, self.nfft, self.hop,
                                             w.ctypes.data_as(C.POINTER(C.c_float)), PDDC_SPEC_PEAK if peak else 0))
        self._h = h

    def process(self, packed, nsamples=None, stream=None) -> int:
        """One batch: a torch uint8 CUDA tensor of packed samples (or a device address with nsamples).  -> the segments
        this batch completed."""
        ptr, nsamples = _packed_arg(self._kind, packed, nsamples)
        L = ddc_lib()
        n = int(L.pddc_spectrum_next_segments(self._h, nsamples))
        check(L.pddc_spectrum_process(self._h, ptr, nsamples, self._stream(stream)))
        return n

    def read(self, clear: bool = False, stream=None):
        """-> (sum float32[nfft], peak float32[nfft] or None, nsegments) accumulated since the last clear"""
        import torch
        dev = torch.device("cuda", self.device)
        s = torch.empty(self.nfft, dtype=torch.float32, device=dev)
        p = torch.empty(self.nfft, dtype=torch.float32, device=dev) if self.peak else None
        n = C.c_uint64()
        check(ddc_lib().pddc_spectrum_read(self._h, s.data_ptr(), p.data_ptr() if self.peak else None, C.byref(n),
                                           1 if clear else 0, self._stream(stream)))
        return s, p, int(n.value)


def spectrum_segments(nfft: int, hop: int, samples_before: int, nsamples: int) -> int:
    """pddc_spectrum_segments: host arithmetic, no device"""
    return int(ddc_lib().pddc_spectrum_segments(nfft, hop, samples_before, nsamples))


def channelizer_prototype(nchan: int, taps_per_branch: int, beta: float = 8.0):
    """A default prototype low-pass for Channelizer: Kaiser-windowed sinc of length taps_per_branch * nchan, cutoff
    fs / (2 nchan) (a channel's half spacing), computed in double, scaled to unity DC gain (sum w = 1) and rounded once
    to float32.  With one tap per branch the sinc's main lobe spans the whole window: the bank then is little more than a
    Kaiser-windowed transform.  -> numpy float32[taps_per_branch * nchan]."""
    import numpy as np
    n = int(nchan) * int(taps_per_branch)
    if n <= 0:
        raise PddcError(-1, "channelizer_prototype: nchan and taps_per_branch must be positive")
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    w = np.sinc(t / nchan) * np.kaiser(n, float(beta))
    return (w / w.sum()).astype(np.float32)


class Channelizer(_StreamObject):
    """pddc_channelizer: all nchan (1024 / 2048 / 4096) equally spaced channels of the packed ADC-rate stream as complex
    time series, from one read of the batch (include/perseus_ddc.h).  proto: the real prototype low-pass, float32 of 1, 2,
    4 or 8 times nchan taps, at most 16384 (channelizer_prototype gives a usable one); hop nchan (default) or nchan/2;
    first / count: the channels (first + i) mod nchan, i < count, that are written (default: all).  The row grid belongs
    to the stream: batches may be cut anywhere on a multiple of 8 samples, and give the same bits.
    set_channels(list) switches to list mode: only the listed channels (1 .. 1024 of them, distinct, any order) are
    written, a row is len(list) values in the list's order, with the bits range mode gives; `channels` holds the list
    (None in range mode) and `count` its length."""
    _kind = "channelizer"

    def __init__(self, nchan: int, proto, hop=None, first: int = 0, count=None, device: int = 0):
        import numpy as np
        self.nchan, self.hop, self.device = int(nchan), int(nchan if hop is None else hop), device
        self.first, self.count = int(first), int(self.nchan if count is None else count)
        self.channels = None
        w = np.ascontiguousarray(np.asarray(proto, dtype=np.float32).reshape(-1))
        self.proto = w
        h = C.c_void_p()
        check(ddc_lib().pddc_channelizer_create(C.byref(h), device, self.nchan, self.hop,
                                                w.ctypes.data_as(C.POINTER(C.c_float)), w.size, self.first, self.count, 0))
        self._h = h

    def next_rows(self, nsamples: int) -> int:
        """rows the next process() of nsamples writes (known from sizes alone)"""
        return int(ddc_lib().pddc_channelizer_next_rows(self._h, nsamples))

    def process(self, packed, nsamples=None, out=None, stream=None):
        """One batch: a torch uint8 CUDA tensor of packed samples (or a device address with nsamples).  -> complex64
        tensor [rows, count] (a view of `out`, a contiguous CUDA tensor of complex64 or float32 pairs, if given)."""
        import torch
        ptr, nsamples = _packed_arg(self._kind, packed, nsamples)
        L = ddc_lib()
        rows = self.next_rows(nsamples) if nsamples % 8 == 0 else 0
        if out is None:
            out = torch.empty((rows, self.count), dtype=torch.complex64, device=torch.device("cuda", self.device))
            cap = rows
        else:
            if not out.is_contiguous():
                raise PddcError(-1, "channelizer: out must be contiguous")
            if out.dtype != torch.complex64:
                out = torch.view_as_complex(out.view(-1, 2))
            out = out.view(-1)
            cap = out.numel() // self.count
        n = C.c_size_t()
        check(L.pddc_channelizer_process(self._h, ptr, nsamples, out.data_ptr() if out.numel() else None, cap,
                                         C.byref(n), self._stream(stream)))
        return out.view(-1)[:n.value * self.count].view(n.value, self.count)

    def set_range(self, first: int, count: int):
        """another channel range (and range mode), from the next process() on"""
        check(ddc_lib().pddc_channelizer_set_range(self._h, first, count))
        self.first, self.count = int(first), int(count)
        self.channels = None

    def set_channels(self, channels):
        """list mode from the next process() on: rows of len(channels) values, out[s, i] = y[s][channels[i]].  A Tuner
        behind this object needs the same list (Tuner.set_channels) before its next batch.  To retune a receiver to a
        channel that is not listed, between two batches: set the union list here and on the Tuner, Tuner.set_freq, then
        (optionally) the shrunk list on both."""
        ch, ptr = _channel_list(channels)
        check(ddc_lib().pddc_channelizer_set_channels(self._h, ptr, ch.size))
        self.channels, self.count = ch, int(ch.size)


def channelizer_rows(nchan: int, hop: int, proto_len: int, samples_before: int, nsamples: int) -> int:
    """pddc_channelizer_rows: host arithmetic, no device"""
    return int(ddc_lib().pddc_channelizer_rows(nchan, hop, proto_len, samples_before, nsamples))


def tuner_prototype(nchan: int, taps_per_branch: int, beta=None):
    """A prototype low-pass for a Channelizer of hop nchan/2 that feeds a Tuner: Kaiser-windowed sinc of length
    taps_per_branch * nchan with its cutoff (-6 dB) at fs / nchan, one channel spacing -- twice channelizer_prototype's,
    which is 6 dB down exactly where a receiver midway between two centres sits.  The pass band then covers half a
    spacing plus the receiver's half width, and the stop band starts where the row rate 2 fs / nchan folds back into
    it (1.5 spacings minus that half width).  beta None: from Kaiser's estimate for a transition of 0.8 spacings,
    A = 14.36 * 0.8 * taps_per_branch + 7.95 dB, beta = 0.1102 (A - 8.7) (A > 50) -- 4.98 / 10.0 for 4 / 8 taps per branch.
    What it reaches for a receiver of half width 0.1 spacings (tests/test_tuner_cpu.py::test_design_helpers computes
    it): the worst-placed receiver (half a spacing off its centre) sees 0.034 dB / 0.0002 dB of pass-band variation with
    4 / 8 taps per branch where channelizer_prototype gives 6.1 / 12.7 dB, and everything that folds into it is 53.7 /
    98.5 dB down (M = 1024; 4096 alike).  Double, sum 1, rounded once.  -> numpy float32[taps_per_branch * nchan]."""
    import numpy as np
    n = int(nchan) * int(taps_per_branch)
    if n <= 0:
        raise PddcError(-1, "tuner_prototype: nchan and taps_per_branch must be positive")
    if beta is None:
        a = 14.36 * 0.8 * taps_per_branch + 7.95
        beta = 0.1102 * (a - 8.7) if a > 50 else 0.5842 * max(a - 21.0, 0.0) ** 0.4 + 0.07886 * max(a - 21.0, 0.0)
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    w = np.sinc(2.0 * t / nchan) * np.kaiser(n, float(beta))
    return (w / w.sum()).astype(np.float32)


def tuner_lowpass(ntaps: int, decim: int, cutoff=None, beta: float = 8.0):
    """The Tuner's common low-pass on rows: Kaiser-windowed sinc of ntaps taps, -6 dB at `cutoff` cycles per row
    (default 0.35 / decim: 70 % of the output rate's Nyquist frequency), double, sum 1, rounded once.
    -> numpy float32[ntaps]."""
    import numpy as np
    ntaps, decim = int(ntaps), int(decim)
    if ntaps <= 0 or decim <= 0:
        raise PddcError(-1, "tuner_lowpass: ntaps and decim must be positive")
    fc = 0.35 / decim if cutoff is None else float(cutoff)
    t = np.arange(ntaps, dtype=np.float64) - (ntaps - 1) / 2.0
    h = np.sinc(2.0 * fc * t) * np.kaiser(ntaps, float(beta))
    return (h / h.sum()).astype(np.float32)


def tuner_outputs(ntaps: int, decim: int, rows_before: int, nrows: int) -> int:
    """pddc_tuner_outputs: host arithmetic, no device"""
    return int(ddc_lib().pddc_tuner_outputs(ntaps, decim, rows_before, nrows))


def tuner_channel_list(nchan: int, freqs):
    """pddc_tuner_channel_list: the distinct channels of the words, ascending -- the list for Channelizer.set_channels
    and Tuner.set_channels; host arithmetic, no device.  -> numpy int32 array"""
    import numpy as np
    f = np.ascontiguousarray(np.asarray(freqs, dtype=np.uint64).reshape(-1) & 0xFFFFFFFF, dtype=np.uint32)
    out = np.empty(max(f.size, 1), dtype=np.int32)
    n = check(ddc_lib().pddc_tuner_channel_list(nchan, f.ctypes.data_as(C.POINTER(C.c_uint32)), f.size,
                                                out.ctypes.data_as(C.POINTER(C.c_int))))
    return out[:n].copy()


def tuner_channel(nchan: int, freg: int):
    """pddc_tuner_channel: (channel, residue) of a 32-bit NCO word; host arithmetic, no device"""
    k, r = C.c_int(), C.c_int32()
    check(ddc_lib().pddc_tuner_channel(nchan, int(freg) & 0xFFFFFFFF, C.byref(k), C.byref(r)))
    return int(k.value), int(r.value)


class Tuner(_StreamObject):
    """pddc_tuner: len(freqs) narrowband receivers behind `channelizer` (its nchan, hop and channel range), each tuned
    with its own 32-bit NCO word (pddc_nco_freg's convention), all filtered by the real low-pass `taps` on rows and
    decimated by `decim`: output rate fs / (hop * decim) (include/perseus_ddc.h).  Feed it every batch of rows the
    Channelizer returns, in order, on the same stream; after Channelizer.set_range call set_range here too, after
    Channelizer.set_channels call set_channels with the same list.  A channelizer in list mode hands its list over at
    construction.  Outputs are bit-identical however the rows are cut into batches, and in either mode.
    Retune to a channel that is not listed, between two batches: set the union list on the Channelizer and here,
    set_freq, then (optionally) the shrunk list on both."""
    _kind = "tuner"

    def __init__(self, channelizer, freqs, taps, decim: int):
        import numpy as np
        ch = channelizer
        self.nchan, self.hop, self.device = ch.nchan, ch.hop, ch.device
        listed = getattr(ch, "channels", None)
        self.first, self.count = (0, ch.nchan) if listed is not None else (ch.first, ch.count)
        self.channels = None
        f = np.ascontiguousarray(np.asarray(freqs, dtype=np.uint64).reshape(-1) & 0xFFFFFFFF, dtype=np.uint32)
        h = np.ascontiguousarray(np.asarray(taps, dtype=np.float32).reshape(-1))
        self.nrx, self.taps, self.decim = int(f.size), h, int(decim)
        hd = C.c_void_p()
        check(ddc_lib().pddc_tuner_create(C.byref(hd), self.device, self.nchan, self.hop, self.first, self.count,
                                          f.ctypes.data_as(C.POINTER(C.c_uint32)), f.size,
                                          h.ctypes.data_as(C.POINTER(C.c_float)), h.size, self.decim, 0))
        self._h = hd
        if listed is not None:                       # created over the full range, then given the list
            self.set_channels(listed)

    def next_outputs(self, nrows: int) -> int:
        """outputs per receiver the next process() of nrows rows writes (known from sizes alone)"""
        return int(ddc_lib().pddc_tuner_next_outputs(self._h, nrows))

    def schedule(self, nrows: int) -> dict:
        """pddc_tuner_schedule: what process() of nrows rows would launch now -- receivers per block, outputs per tile,
        outputs per run, blocks along the outputs, rows carried afterwards.  Launches nothing, moves no counter."""
        o = (C.c_int * 5)()
        check(ddc_lib().pddc_tuner_schedule(self._h, nrows, o))
        return {"group": o[0], "tile": o[1], "run": o[2], "blocks": o[3], "carried": o[4]}

    def process(self, rows, nrows=None, out=None, stream=None):
        """One batch of rows: the complex64 CUDA tensor [nrows, count] Channelizer.process returned (or a device
        address with nrows).  -> complex64 [nrx, outputs] (a view of `out`, a contiguous CUDA tensor [nrx, capacity] of
        complex64, if given: receiver j's series starts at out[j, 0])."""
        import torch
        if hasattr(rows, "data_ptr"):
            if not rows.is_contiguous():
                raise PddcError(-1, "tuner: rows must be contiguous")
            if nrows is None:
                nrows = (rows.numel() if rows.dtype == torch.complex64 else rows.numel() // 2) // self.count
            ptr = rows.data_ptr() if nrows else None
        else:
            ptr = int(rows)
            if nrows is None:
                raise PddcError(-1, "tuner: a device address needs nrows")
        n_due = self.next_outputs(nrows)
        if out is None:
            out = torch.empty((self.nrx, n_due), dtype=torch.complex64, device=torch.device("cuda", self.device))
        elif out.dtype != torch.complex64 or out.dim() != 2 or out.shape[0] != self.nrx or not out.is_contiguous():
            raise PddcError(-1, "tuner: out must be a contiguous complex64 tensor [nrx, capacity]")
        n = C.c_size_t()
        check(ddc_lib().pddc_tuner_process(self._h, ptr, nrows, out.data_ptr() if out.numel() else None, out.shape[1],
                                           C.byref(n), self._stream(stream)))
        return out[:, :n.value]

    def set_freq(self, rx: int, freg: int):
        """retune receiver rx from the next row on; the phase accumulator goes on without a step"""
        check(ddc_lib().pddc_tuner_set_freq(self._h, rx, int(freg) & 0xFFFFFFFF))

    def set_range(self, first: int, count: int):
        """the Channelizer's new range (Channelizer.set_range), from the next process() on"""
        check(ddc_lib().pddc_tuner_set_range(self._h, first, count))
        self.first, self.count = int(first), int(count)
        self.channels = None

    def set_channels(self, channels):
        """the Channelizer's list (Channelizer.set_channels), from the next process() on: rows of len(channels) values in
        this order.  Every receiver's channel must be listed; in list mode set_freq to an unlisted channel is refused
        (the retune sequence: the class docstring)."""
        ch, ptr = _channel_list(channels)
        check(ddc_lib().pddc_tuner_set_channels(self._h, ptr, ch.size))
        self.channels, self.first, self.count = ch, 0, int(ch.size)


def rxfilter_tile_outputs() -> int:
    """pddc_rxfilter_tile_outputs: outputs per tile of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_rxfilter_tile_outputs())


def rxfilter_bank(rate_hz: float, half_widths_hz, ntaps: int, beta: float = 8.0):
    """A bank for RxFilter: one Kaiser-windowed sinc of ntaps taps per half width, -6 dB at half_width Hz of a series at
    rate_hz (tuner_lowpass's formula with fc = half_width / rate_hz), double, sum 1, rounded once.  All rows have the
    delay (ntaps - 1) / 2.  A half width <= 0 or >= rate_hz / 2 is refused.  -> numpy float32[len(half_widths_hz), ntaps]."""
    import numpy as np
    ntaps, rate = int(ntaps), float(rate_hz)
    w = np.asarray(half_widths_hz, dtype=np.float64).reshape(-1)
    if ntaps <= 0 or not rate > 0.0 or w.size == 0:
        raise PddcError(-1, "rxfilter_bank: ntaps, the rate and the number of half widths must be positive")
    if not np.all((w > 0.0) & (w < 0.5 * rate)):
        raise PddcError(-1, "rxfilter_bank: every half width must lie in (0, rate / 2)")
    t = np.arange(ntaps, dtype=np.float64) - (ntaps - 1) / 2.0
    win = np.kaiser(ntaps, float(beta))
    rows = [np.sinc(2.0 * (hw / rate) * t) * win for hw in w]
    return np.stack([(h / h.sum()).astype(np.float32) for h in rows])


class RxFilter(_StreamObject):
    """pddc_rxfilter: every receiver's complex series, such as Tuner.process returns, through one of a bank of real FIR
    filters -- each receiver its own bandwidth -- one output per input, on the device (include/perseus_ddc.h).  bank:
    float32 [B, T] (rxfilter_bank), sel: one filter index per receiver.  It goes between Tuner and Demod.  Feed it
    every batch in order on one stream; outputs are bit-identical however the series is cut."""
    _kind = "rxfilter"

    def __init__(self, bank, sel, device: int = 0):
        import numpy as np
        b = np.asarray(bank, dtype=np.float32)
        if b.ndim != 2:
            raise PddcError(-1, "rxfilter: the bank must be a float32 array [filters, taps]")
        b = np.ascontiguousarray(b)
        s = np.ascontiguousarray(np.asarray(sel, dtype=np.int64).reshape(-1).clip(-1, 1 << 30), dtype=np.int32)
        self.bank, self.nrx, self.device = b, int(s.size), device
        self.nfilters, self.taps = int(b.shape[0]), int(b.shape[1])
        h = C.c_void_p()
        check(ddc_lib().pddc_rxfilter_create(C.byref(h), device, self.nrx, b.ctypes.data_as(C.POINTER(C.c_float)),
                                             self.nfilters, self.taps, s.ctypes.data_as(C.POINTER(C.c_int))))
        self._h = h

    def process(self, z, out=None, stream=None):
        """One batch: a complex64 CUDA tensor [nrx, n] whose rows are contiguous (any row stride: the view Tuner.process
        returns is fine).  -> complex64 [nrx, n] (a view of `out`, a complex64 CUDA tensor [nrx, capacity] with contiguous
        rows, if given).  `out` must not overlap z."""
        import torch
        if not self._rows(z, torch.complex64):
            raise PddcError(-1, "rxfilter: z must be a complex64 tensor [nrx, n] with contiguous rows")
        n = int(z.shape[1])
        out, cap = self._out(out, n, torch.complex64, "out must be a complex64")
        check(ddc_lib().pddc_rxfilter_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)),
                                              out.data_ptr() if out.numel() else None, cap, self._stream(stream)))
        return out[:, :n]

    def set_rx(self, rx: int, filter: int):
        """receiver rx from the next output on: the bank's filter `filter` over the same inputs, the carried ones
        included -- nothing is reset"""
        check(ddc_lib().pddc_rxfilter_set_rx(self._h, int(rx), int(filter)))


PDDC_DEMOD_AM, PDDC_DEMOD_FM, PDDC_DEMOD_SSB = 0, 1, 2
PDDC_DEMOD_DCBLOCK, PDDC_DEMOD_AGC = 0x1, 0x2


def demod_tile_outputs() -> int:
    """pddc_demod_tile_outputs: outputs per tile of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_demod_tile_outputs())


def demod_ssb_words(fs: float, out_rate: float, carrier_hz: float, lo_hz: float, hi_hz: float, upper: bool = True):
    """The two words of a single-sideband receiver for the audio band lo_hz .. hi_hz above (upper) or below the carrier:
    the Tuner's word, tuned to the middle of that sideband (pddc_nco_freg's rule on fs, the ADC rate), and the BFO word
    of Demod at out_rate, which moves the sideband back: an audio tone f comes out of the tuner at f - (lo + hi) / 2
    (upper) or (lo + hi) / 2 - f (lower), and the phasor exp(-2 pi i bfo m / 2^32) puts it at +f or -f, whose real part
    is the tone.  Give the Tuner's low-pass the half width (hi - lo) / 2.  CW is a narrow band around the wanted pitch.
    -> (tuner word, bfo), both in 0 .. 2^32 - 1."""
    mid = 0.5 * (float(lo_hz) + float(hi_hz))
    sign = 1.0 if upper else -1.0
    word = int((float(carrier_hz) + sign * mid) / float(fs) * 4294967296.0) & 0xFFFFFFFF
    bfo = int(round(-sign * mid / float(out_rate) * 4294967296.0)) & 0xFFFFFFFF
    return word, bfo


class Demod(_StreamObject):
    """pddc_demod: AM, FM and SSB audio from complex series such as Tuner.process returns, one real float32 output per
    input, on the device (include/perseus_ddc.h).  rx: one (mode, bfo, flags) per receiver -- mode PDDC_DEMOD_AM / _FM /
    _SSB, bfo the 32-bit BFO word of SSB (demod_ssb_words), flags PDDC_DEMOD_DCBLOCK | PDDC_DEMOD_AGC.  rho (DC block
    pole), lam (AGC envelope decay per output), target and gmax (AGC level and largest gain) are common to all
    receivers.  Feed it every batch in order on one stream; outputs are bit-identical however the series is cut."""
    _kind = "demod"

    def __init__(self, rx, device: int = 0, rho: float = 0.995, lam: float = 0.9995, target: float = 0.25,
                 gmax: float = 1.0e4):
        rx = [tuple(r) for r in rx]
        self.nrx, self.device = len(rx), device
        arr = (DemodRx * max(self.nrx, 1))()
        for j, (mode, bfo, flags) in enumerate(rx):
            arr[j] = DemodRx(int(mode), int(bfo) & 0xFFFFFFFF, int(flags) & 0xFFFFFFFF)
        self.params = DemodParams(rho, lam, target, gmax)
        h = C.c_void_p()
        check(ddc_lib().pddc_demod_create(C.byref(h), device, self.nrx, arr, C.byref(self.params)))
        self._h = h

    def process(self, z, out=None, stream=None):
        """One batch: a complex64 CUDA tensor [nrx, n] whose rows are contiguous (any row stride: the view Tuner.process
        returns is fine).  -> float32 [nrx, n] (a view of `out`, a float32 CUDA tensor [nrx, capacity] with contiguous
        rows, if given)."""
        import torch
        if not self._rows(z, torch.complex64):
            raise PddcError(-1, "demod: z must be a complex64 tensor [nrx, n] with contiguous rows")
        n = int(z.shape[1])
        out, cap = self._out(out, n, torch.float32, "out must be a float32")
        check(ddc_lib().pddc_demod_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)),
                                           out.data_ptr() if out.numel() else None, cap, self._stream(stream)))
        return out[:, :n]

    def set_rx(self, rx: int, mode: int, bfo: int = 0, flags: int = 0):
        """receiver rx from the next output on: another word alone goes on phase-continuously, another mode or other
        flags start that receiver's carried values afresh"""
        check(ddc_lib().pddc_demod_set_rx(self._h, rx, int(mode), int(bfo) & 0xFFFFFFFF, int(flags) & 0xFFFFFFFF))


PDDC_CARRIER_OFF, PDDC_CARRIER_DSB, PDDC_CARRIER_USB, PDDC_CARRIER_LSB = 0, 1, 2, 3


def carrier_tile_outputs() -> int:
    """pddc_carrier_tile_outputs: outputs per tile of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_carrier_tile_outputs())


def carrier_group() -> int:
    """pddc_carrier_group: receivers per block of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_carrier_group())


def carrier_loop(bandwidth_hz: float, rate_hz: float, damping: float = 0.7071):
    """The gains of Carrier's loop for a natural frequency of bandwidth_hz at rate_hz outputs per second:
    wn = 2 pi bandwidth / rate, kp = 2 damping wn, ki = wn^2.  -> (kp, ki)"""
    wn = 2.0 * math.pi * float(bandwidth_hz) / float(rate_hz)
    return 2.0 * float(damping) * wn, wn * wn


def carrier_hilbert(L: int, beta: float = 8.0):
    """The Hilbert filter of Carrier's USB / LSB: L taps (odd), the type-III ideal 2 / (pi (k - D)) at odd k - D and 0 at
    even, D = (L - 1) / 2, under a Kaiser window.  -> float32 [L]"""
    import numpy as np
    L = int(L)
    if L < 3 or not L & 1:
        raise ValueError("carrier_hilbert: L odd, >= 3")
    k = np.arange(L, dtype=np.int64) - (L - 1) // 2
    odd = (k & 1) != 0
    h = np.where(odd, 2.0 / (np.pi * np.where(odd, k, 1)), 0.0) * np.kaiser(L, beta)
    return h.astype(np.float32)


def carrier_status_dtype():
    """pddc_carrier_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("theta", np.uint32), ("freq", np.float32), ("err", np.float32), ("locked", np.uint32)])


class Carrier(_StreamObject):
    """pddc_carrier: synchronous AM -- a phase-locked loop on each receiver's carrier, on the device
    (include/perseus_ddc.h).  It goes between RxFilter (or Tuner) and Demod: z, rotated by the loop's phasor, comes out
    as a complex series whose real part is the audio of both sidebands (PDDC_CARRIER_DSB) or, through the Hilbert filter
    `hilbert` (carrier_hilbert), of the upper or the lower one (_USB / _LSB, delayed by (L - 1) / 2 outputs); Demod in
    PDDC_DEMOD_SSB with word 0 takes that real part and adds DC block and AGC.  rx: one (mode, kp, ki) per receiver
    (carrier_loop gives the gains), PDDC_CARRIER_OFF passes z.  vmax bounds the loop's frequency term (half-turns per
    output), gamma smooths the lock metric, a receiver is locked while that metric is below lock_thr.  Feed it every
    batch in order on one stream; outputs are bit-identical however the series is cut."""
    _kind = "carrier"

    def __init__(self, rx, hilbert, vmax: float = 0.25, gamma: float = 1.0 / 64, lock_thr: float = 0.05, device: int = 0):
        import numpy as np
        rx = [tuple(r) for r in rx]
        self.nrx, self.device = len(rx), device
        arr = (CarrierRx * max(self.nrx, 1))()
        for j, (mode, kp, ki) in enumerate(rx):
            arr[j] = CarrierRx(_clip(mode), float(kp), float(ki))
        h = np.ascontiguousarray(hilbert, dtype=np.float32).reshape(-1)
        self.ntaps = int(h.size)
        self.params = CarrierParams(vmax, gamma, lock_thr)
        hd = C.c_void_p()
        check(ddc_lib().pddc_carrier_create(C.byref(hd), device, self.nrx, C.byref(self.params), arr,
                                            h.ctypes.data_as(C.POINTER(C.c_float)), _clip(h.size)))
        self._h = hd

    def process(self, z, out=None, stream=None):
        """One batch: a complex64 CUDA tensor [nrx, n] whose rows are contiguous (any row stride).  -> complex64 [nrx, n]
        (a view of `out`, a complex64 CUDA tensor [nrx, capacity] with contiguous rows, if given; `out` may be z itself:
        in place)."""
        import torch
        if not self._rows(z, torch.complex64):
            raise PddcError(-1, "carrier: z must be a complex64 tensor [nrx, n] with contiguous rows")
        n = int(z.shape[1])
        out, cap = self._out(out, n, torch.complex64, "out must be a complex64")
        check(ddc_lib().pddc_carrier_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)),
                                             out.data_ptr() if out.numel() else None, cap, self._stream(stream)))
        return out[:, :n]

    def set_rx(self, rx: int, mode: int, kp: float, ki: float):
        """receiver rx from the next output on: other gains alone leave the loop running, another mode starts that
        receiver's loop and history afresh"""
        check(ddc_lib().pddc_carrier_set_rx(self._h, int(rx), _clip(mode), float(kp), float(ki)))

    def read(self, stream=None):
        """-> numpy structured array [nrx] (theta, freq, err, locked) after the batches submitted so far (it waits for
        them); the carrier's offset from the tuned frequency is freq * rate / 2 Hz.  A receiver just created, reset or
        given another mode, and an OFF one, has err = 0 and reads as locked: err says something after some 1 / gamma
        outputs"""
        import numpy as np
        st = np.zeros(self.nrx, dtype=carrier_status_dtype())
        check(ddc_lib().pddc_carrier_read(self._h, st.ctypes.data, self._stream(stream)))
        return st


PDDC_SQL_GATE, PDDC_SQL_RELATIVE = 0x1, 0x2


def squelch_tile_outputs() -> int:
    """pddc_squelch_tile_outputs: samples per tile of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_squelch_tile_outputs())


def squelch_blocks(block: int, samples_before: int, n: int) -> int:
    """pddc_squelch_blocks: blocks of `block` samples that n samples after samples_before complete,
    (before + n) // block - before // block; 0 for an unsupported block length; host arithmetic, no device"""
    block = int(block)
    return int(ddc_lib().pddc_squelch_blocks(block if -1 << 31 <= block < 1 << 31 else 0, samples_before, n))


def squelch_status_dtype():
    """pddc_squelch_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("level", np.float32), ("floor", np.float32), ("peak", np.float32), ("open", np.uint32),
                     ("opens", np.uint32)])


class Squelch(_StreamObject):
    """pddc_squelch: a level meter and a gate per receiver, on the device (include/perseus_ddc.h).  It goes between
    Demod and Audio and reads the complex series Demod reads together with Demod's audio: the mean power of every
    `block` samples is a level; a receiver opens after `attack` consecutive blocks at or above its open threshold and
    closes after `hang` consecutive blocks below its close threshold; the audio is passed through a linear gain ramp of
    `ramp` samples.  rx: one (open_thr, close_thr, flags) per receiver, flags PDDC_SQL_GATE (without it the audio passes
    ungated and the receiver is metered only) | PDDC_SQL_RELATIVE (the thresholds are factors of the receiver's noise
    floor, the smallest level seen while closed, which rises by the factor `up` per block).  Feed it every batch in
    order on one stream; all outputs are bit-identical however the series is cut."""
    _kind = "squelch"

    def __init__(self, rx, block: int, attack: int, hang: int, ramp: int, up: float = 1.0, device: int = 0):
        rx = [tuple(r) for r in rx]
        self.nrx, self.device = len(rx), device
        arr = (SquelchRx * max(self.nrx, 1))()
        for j, (open_thr, close_thr, flags) in enumerate(rx):
            arr[j] = SquelchRx(float(open_thr), float(close_thr), int(flags) & 0xFFFFFFFF)
        self.block, self.attack, self.hang, self.ramp, self.up = int(block), int(attack), int(hang), int(ramp), float(up)
        self.params = SquelchParams(_clip(block), _clip(attack), _clip(hang), _clip(ramp), up)
        h = C.c_void_p()
        check(ddc_lib().pddc_squelch_create(C.byref(h), device, self.nrx, C.byref(self.params), arr))
        self._h = h

    def next_blocks(self, n: int) -> int:
        """blocks per receiver the next process() of n samples completes (known from sizes alone)"""
        c = C.c_size_t()
        check(ddc_lib().pddc_squelch_next_blocks(self._h, n, C.byref(c)))
        return int(c.value)

    def process(self, z, a, out=None, levels=None, states=None, stream=None):
        """One batch: z a complex64 and a a float32 CUDA tensor [nrx, n] whose rows are contiguous (any row stride: the
        views Tuner.process and Demod.process return are fine).  -> (out float32 [nrx, n], levels float32 [nrx, blocks],
        states uint8 [nrx, blocks]): views of `out`, `levels`, `states`, CUDA tensors [nrx, capacity] with contiguous
        rows, if given; levels and states must then have the same row stride.  `out` may be `a` itself (gating in place);
        it must not overlap z or a otherwise."""
        import torch
        if not self._rows(z, torch.complex64) or not self._rows(a, torch.float32) or a.shape[1] != z.shape[1]:
            raise PddcError(-1, "squelch: z must be a complex64 and a a float32 tensor [nrx, n] with contiguous rows")
        n = int(z.shape[1])
        due = self.next_blocks(n)
        out, cap = self._out(out, n, torch.float32, "out must be a float32")
        # one row stride for both: one that is not given gets the other's
        both = "levels must be a float32 and states a uint8"
        dev = torch.device("cuda", self.device)
        if levels is None and states is not None:
            levels = torch.empty((self.nrx, int(states.stride(0))), dtype=torch.float32, device=dev)
        elif states is None and levels is not None:
            states = torch.empty((self.nrx, int(levels.stride(0))), dtype=torch.uint8, device=dev)
        levels, lcap = self._out(levels, due, torch.float32, both)
        states, _ = self._out(states, due, torch.uint8, both)
        if due and self.nrx > 1 and levels.stride(0) != states.stride(0):
            raise PddcError(-1, "squelch: levels and states must have the same row stride")
        # the shorter of the two is the capacity when one is too short, levels' stride otherwise
        bcap = lcap if states.shape[1] >= due else min(int(levels.shape[1]), int(states.shape[1]))
        c = C.c_size_t()
        check(ddc_lib().pddc_squelch_process(self._h, z.data_ptr() if n else None, a.data_ptr() if n else None, n,
                                             int(z.stride(0)), int(a.stride(0)), out.data_ptr() if out.numel() else None, cap,
                                             levels.data_ptr() if levels.numel() else None,
                                             states.data_ptr() if states.numel() else None, bcap, C.byref(c),
                                             self._stream(stream)))
        return out[:, :n], levels[:, :c.value], states[:, :c.value]

    def set_rx(self, rx: int, open_thr: float, close_thr: float, flags: int = 0):
        """receiver rx: the thresholds from the next block end on, the flags from the next sample on; nothing carried
        is reset"""
        check(ddc_lib().pddc_squelch_set_rx(self._h, int(rx), float(open_thr), float(close_thr), int(flags) & 0xFFFFFFFF))

    def read(self, clear_peak: bool = False, stream=None):
        """-> numpy structured array [nrx] (level, floor, peak, open, opens) after the batches submitted so far (it
        waits for them); clear_peak: peak restarts at 0 for the blocks that complete after the call"""
        import numpy as np
        st = np.zeros(self.nrx, dtype=squelch_status_dtype())
        check(ddc_lib().pddc_squelch_read(self._h, st.ctypes.data, 1 if clear_peak else 0, self._stream(stream)))
        return st


PDDC_ADAPT_OFF, PDDC_ADAPT_NR, PDDC_ADAPT_NOTCH = 0, 1, 2
PDDC_ADAPT_RESTART = 0x1


def adapt_tile_outputs() -> int:
    """pddc_adapt_tile_outputs: samples per tile of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_adapt_tile_outputs())


class Adapt(_StreamObject):
    """pddc_adapt: automatic notch and noise reduction per receiver, on the device (include/perseus_ddc.h).  It goes
    between Squelch (or Demod) and Audio: a leaky normalised LMS predictor of `taps` taps (16, 32, 64, 128) over the audio
    delayed by `delay` samples (1 .. 256); what it predicts is the noise-reduced audio (PDDC_ADAPT_NR), what it cannot
    predict is the audio with carrier whistles removed (PDDC_ADAPT_NOTCH); PDDC_ADAPT_OFF passes the audio and holds the
    weights.  rx: one (mode, mu, leak) per receiver, the step 0 < mu < 2 and the leak 0 <= leak < 1.  Feed it every
    batch in order on one stream; all outputs are bit-identical however the series is cut."""
    _kind = "adapt"

    def __init__(self, rx, taps: int, delay: int, eps: float = 1.0e-6, device: int = 0):
        rx = [tuple(r) for r in rx]
        self.nrx, self.device = len(rx), device
        arr = (AdaptRx * max(self.nrx, 1))()
        for j, r in enumerate(rx):
            mode, mu, leak = r[:3]
            arr[j] = AdaptRx(int(mode) & 0xFFFFFFFF, float(mu), float(leak), (int(r[3]) if len(r) > 3 else 0) & 0xFFFFFFFF)
        self.taps, self.delay, self.eps = int(taps), int(delay), float(eps)
        self.params = AdaptParams(_clip(taps), _clip(delay), eps)
        h = C.c_void_p()
        check(ddc_lib().pddc_adapt_create(C.byref(h), device, self.nrx, C.byref(self.params), arr))
        self._h = h

    def process(self, a, out=None, stream=None):
        """One batch: a float32 CUDA tensor [nrx, n] whose rows are contiguous (any row stride: the views Demod.process
        and Squelch.process return are fine).  -> float32 [nrx, n] (a view of `out`, a float32 CUDA tensor [nrx,
        capacity] with contiguous rows, if given).  `out` may be `a` itself (in place); it must not overlap a
        otherwise."""
        import torch
        if not self._rows(a, torch.float32):
            raise PddcError(-1, "adapt: a must be a float32 tensor [nrx, n] with contiguous rows")
        n = int(a.shape[1])
        out, cap = self._out(out, n, torch.float32, "out must be a float32")
        check(ddc_lib().pddc_adapt_process(self._h, a.data_ptr() if n else None, n, int(a.stride(0)),
                                           out.data_ptr() if out.numel() else None, cap, self._stream(stream)))
        return out[:, :n]

    def set_rx(self, rx: int, mode: int, mu: float, leak: float, flags: int = 0):
        """receiver rx from the next sample on; the weights are kept unless flags has PDDC_ADAPT_RESTART"""
        check(ddc_lib().pddc_adapt_set_rx(self._h, int(rx), int(mode) & 0xFFFFFFFF, float(mu), float(leak), int(flags) & 0xFFFFFFFF))

    def read_weights(self, stream=None):
        """-> numpy float32 [nrx, taps]: the weights as the last batch left them (it waits for it)"""
        import numpy as np
        w = np.zeros((self.nrx, self.taps), dtype=np.float32)
        check(ddc_lib().pddc_adapt_read_weights(self._h, w.ctypes.data, self._stream(stream)))
        return w


PDDC_DENOISE_OFF, PDDC_DENOISE_NR = 0, 1
PDDC_DENOISE_RESTART, PDDC_DENOISE_HOLD = 0x1, 0x2


def denoise_delay(nfft: int) -> int:
    """pddc_denoise_delay: the stage's delay in samples (nfft); host arithmetic, no device"""
    return int(ddc_lib().pddc_denoise_delay(_clip(nfft)))


def denoise_tile_frames() -> int:
    """pddc_denoise_tile_frames: frames per block pass of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_denoise_tile_frames())


def denoise_window(nfft: int, hop: int):
    """The square-root Hann window sqrt(0.5 - 0.5 cos(2 pi (i + 0.5) / nfft)), scaled so that the squares of the nfft / hop
    windows that meet at a sample sum to 1: with it unity gain (PDDC_DENOISE_OFF) gives the delayed input.  -> float64 (the object takes it as float32)"""
    import numpy as np
    i = np.arange(nfft, dtype=np.float64)
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 0.5) / nfft))
    return w / np.sqrt(nfft / (2.0 * hop))


class Denoise(_StreamObject):
    """pddc_denoise: spectral noise reduction per receiver, on the device (include/perseus_ddc.h).  It goes where Adapt
    goes, between Demod (or Squelch, or Adapt) and Audio: frames of `nfft` (256, 512, 1024) samples every `hop` (nfft/2,
    nfft/4), a tracked noise estimate and a decision-directed gain per bin, overlap-add; the output is the input delayed
    by nfft samples with the noise taken down to the gain floor.  rx: one (mode, beta, gmin, alpha[, flags]) per
    receiver, or a count for the defaults.  Feed it every batch in order on one stream; all outputs are bit-identical
    however the series is cut."""
    _kind = "denoise"

    def __init__(self, rx, nfft: int = 256, hop: int = 128, window=None, smooth: float = 0.3, up: float = 0.02,
                 down: float = 0.3, nmin: float = 1.0e-4, eps: float = 1.0e-20, device: int = 0):
        import numpy as np
        if isinstance(rx, int):
            rx = [(PDDC_DENOISE_NR, 2.0, 0.1, 0.98)] * rx
        rx = [tuple(r) for r in rx]
        self.nrx, self.device = len(rx), device
        arr = (DenoiseRx * max(self.nrx, 1))()
        for j, r in enumerate(rx):
            mode, beta, gmin, alpha = r[:4]
            arr[j] = DenoiseRx(int(mode) & 0xFFFFFFFF, float(beta), float(gmin), float(alpha),
                               (int(r[4]) if len(r) > 4 else 0) & 0xFFFFFFFF)
        self.nfft, self.hop = int(nfft), int(hop)
        self.params = DenoiseParams(_clip(nfft), _clip(hop), smooth, up, down, nmin, eps)
        if window is None:
            window = denoise_window(self.nfft, self.hop)
        w = np.ascontiguousarray(window, dtype=np.float32)
        if w.shape != (self.nfft,):
            raise PddcError(-1, "denoise: window must hold nfft values")
        h = C.c_void_p()
        check(ddc_lib().pddc_denoise_create(C.byref(h), device, self.nrx, C.byref(self.params), w.ctypes.data, arr))
        self._h = h

    def process(self, x, out=None, stream=None):
        """One batch: a float32 CUDA tensor [nrx, n] whose rows are contiguous (any row stride: the views Demod.process,
        Squelch.process and Adapt.process return are fine).  -> float32 [nrx, n] (a view of `out`, a float32 CUDA tensor
        [nrx, capacity] with contiguous rows, if given): the input nfft samples ago, denoised.  `out` must not overlap x."""
        import torch
        if not self._rows(x, torch.float32):
            raise PddcError(-1, "denoise: x must be a float32 tensor [nrx, n] with contiguous rows")
        n = int(x.shape[1])
        out, cap = self._out(out, n, torch.float32, "out must be a float32")
        check(ddc_lib().pddc_denoise_process(self._h, x.data_ptr() if n else None, n, int(x.stride(0)),
                                             out.data_ptr() if out.numel() else None, cap, self._stream(stream)))
        return out[:, :n]

    def set_rx(self, rx: int, mode: int, beta: float, gmin: float, alpha: float, flags: int = 0):
        """receiver rx, for every frame whose last sample arrives in a later batch.  flags: PDDC_DENOISE_RESTART (the next
        completed frame is a first frame), PDDC_DENOISE_HOLD (the noise estimate stays, until a call without it)"""
        check(ddc_lib().pddc_denoise_set_rx(self._h, int(rx), int(mode) & 0xFFFFFFFF, float(beta), float(gmin), float(alpha),
                                            int(flags) & 0xFFFFFFFF))

    def read_noise(self, stream=None):
        """-> numpy float32 [nrx, nfft/2 + 1]: the noise estimate N as the last batch left it (it waits for it)"""
        import numpy as np
        nn = np.zeros((self.nrx, self.nfft // 2 + 1), dtype=np.float32)
        check(ddc_lib().pddc_denoise_read_noise(self._h, nn.ctypes.data, self._stream(stream)))
        return nn


PDDC_EQ_MAX_SECTIONS = 8
PDDC_EQ_RESTART = 0x1
(PDDC_EQ_LOWPASS, PDDC_EQ_HIGHPASS, PDDC_EQ_BANDPASS, PDDC_EQ_NOTCH, PDDC_EQ_PEAK, PDDC_EQ_LOWSHELF, PDDC_EQ_HIGHSHELF,
 PDDC_EQ_LOWPASS1, PDDC_EQ_HIGHPASS1) = range(9)


def eq_tile_outputs() -> int:
    """pddc_eq_tile_outputs: samples per tile of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_eq_tile_outputs())


def eq_section(kind: int, rate_hz: float, f_hz: float, q: float = 0.7071, gain_db: float = 0.0) -> EqSection:
    """pddc_eq_design: one second-order section in double -- the RBJ cookbook's PDDC_EQ_LOWPASS, _HIGHPASS, _BANDPASS (0 dB
    peak), _NOTCH, _PEAK, _LOWSHELF, _HIGHSHELF, and the one-pole _LOWPASS1 / _HIGHPASS1 (half power at f_hz; q and
    gain_db are not used).  Host arithmetic, no device."""
    s = EqSection()
    check(ddc_lib().pddc_eq_design(_clip(kind), float(rate_hz), float(f_hz), float(q), float(gain_db), C.byref(s)))
    return s


def eq_deemphasis(rate_hz: float, tau_s: float) -> EqSection:
    """the FM de-emphasis of time constant tau_s (50e-6, 75e-6; narrow-band FM: 750e-6 or so): PDDC_EQ_LOWPASS1 at 1 / (2 pi tau)"""
    import math
    tau = float(tau_s)
    return eq_section(PDDC_EQ_LOWPASS1, rate_hz, 1.0 / (2.0 * math.pi * tau) if tau > 0.0 else float("nan"))


def eq_response(sections, rate_hz: float, freqs):
    """H(f) of a cascade at the frequencies `freqs` (Hz): the product of (b0 + b1 z^-1 + b2 z^-2) / (1 + a1 z^-1 + a2 z^-2),
    z = exp(2 pi j f / rate_hz), over `sections` (EqSection or five values each).  -> numpy complex128, the shape of
    freqs.  For a display and the tests; numpy, no device."""
    import numpy as np
    f = np.asarray(freqs, dtype=np.float64)
    z1 = np.exp(-2j * np.pi * f / float(rate_hz))
    z2 = z1 * z1
    h = np.ones(f.shape, dtype=np.complex128)
    for s in sections:
        b0, b1, b2, a1, a2 = (float(v) for v in s)
        h = h * ((b0 + b1 * z1 + b2 * z2) / (1.0 + a1 * z1 + a2 * z2))
    return h


def _eq_sections(sections):
    """a cascade as the C ABI takes it: EqSection or five values each -> (count, array of at least one)"""
    secs = [s if isinstance(s, EqSection) else EqSection(*(float(v) for v in s)) for s in sections]
    return len(secs), (EqSection * max(len(secs), 1))(*secs)


class Eq(_StreamObject):
    """pddc_eq: an equaliser per receiver, on the device (include/perseus_ddc.h).  It goes behind Demod, Squelch, Adapt or
    Denoise and in front of Audio (or behind Audio, at 48 kHz): a cascade of up to `sections` (1, 2, 4, 8) second-order
    sections per receiver -- de-emphasis, a CW peak filter, notches, shelves, high and low cut (eq_section, eq_deemphasis)
    -- in binary64 arithmetic on float32 audio.  rx: one list of sections (EqSection or (b0, b1, b2, a1, a2)) per
    receiver; an empty list passes the audio word for word.  Feed it every batch in order on one stream; all outputs are
    bit-identical however the series is cut, and whatever `sections` is."""
    _kind = "eq"

    def __init__(self, rx, sections: int = 4, device: int = 0):
        rx = [list(r) for r in rx]
        self.nrx, self.device, self.sections = len(rx), device, int(sections)
        S = self.sections if self.sections in (1, 2, 4, 8) else 0
        nsec = (C.c_int * max(self.nrx, 1))()
        sec = (EqSection * max(self.nrx * max(S, 1), 1))()
        for j, r in enumerate(rx):
            nsec[j] = _clip(len(r))
            for s, c in enumerate(r[:S]):
                sec[j * S + s] = c if isinstance(c, EqSection) else EqSection(*(float(v) for v in c))
        self.params = EqParams(_clip(sections))
        h = C.c_void_p()
        check(ddc_lib().pddc_eq_create(C.byref(h), device, self.nrx, C.byref(self.params), nsec, sec))
        self._h = h

    def process(self, a, out=None, stream=None):
        """One batch: a float32 CUDA tensor [nrx, n] whose rows are contiguous (any row stride: the views Demod.process,
        Squelch.process, Adapt.process and Denoise.process return are fine).  -> float32 [nrx, n] (a view of `out`, a
        float32 CUDA tensor [nrx, capacity] with contiguous rows, if given).  `out` may be `a` itself (in place); it must
        not overlap a otherwise."""
        import torch
        if not self._rows(a, torch.float32):
            raise PddcError(-1, "eq: a must be a float32 tensor [nrx, n] with contiguous rows")
        n = int(a.shape[1])
        out, cap = self._out(out, n, torch.float32, "out must be a float32")
        check(ddc_lib().pddc_eq_process(self._h, a.data_ptr() if n else None, n, int(a.stride(0)),
                                        out.data_ptr() if out.numel() else None, cap, self._stream(stream)))
        return out[:, :n]

    def set_rx(self, rx: int, sections, flags: int = 0):
        """receiver rx's cascade from the next sample on; the states are kept unless flags has PDDC_EQ_RESTART"""
        n, arr = _eq_sections(sections)
        check(ddc_lib().pddc_eq_set_rx(self._h, int(rx), _clip(n), arr, int(flags) & 0xFFFFFFFF))

    def read_state(self, stream=None):
        """-> numpy float64 [nrx, sections, 2]: s1, s2 as the last batch left them (it waits for it)"""
        import numpy as np
        st = np.zeros((self.nrx, self.sections, 2), dtype=np.float64)
        check(ddc_lib().pddc_eq_read_state(self._h, st.ctypes.data, self._stream(stream)))
        return st


PDDC_NB_ON = 0x1


def blanker_tile_outputs() -> int:
    """pddc_blanker_tile_outputs: samples per tile of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_blanker_tile_outputs())


def blanker_status_dtype():
    """pddc_blanker_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("ref", np.float32), ("triggers", np.uint32), ("blanked", np.uint32)])


class Blanker(_StreamObject):
    """pddc_blanker: an impulse noise blanker per receiver, on the device (include/perseus_ddc.h).  It goes between Tuner
    and RxFilter, where an impulse is still a few samples long: the mean power of every `block` samples moves a
    reference (smoothing `beta`, at most the factor `cap` up per block); a sample whose power exceeds the reference times
    the receiver's threshold is a trigger; the output is the input delayed by `delay` = guard + ramp samples, zero
    within `guard` samples of a trigger and brought back through a linear ramp of `ramp` samples on either side.  rx: one
    (thr, flags) per receiver, flags PDDC_NB_ON (without it the receiver is delayed and metered only).  Feed it every
    batch in order on one stream; all outputs are bit-identical however the series is cut.  The last `delay` inputs
    of a stream come out when `delay` more samples are fed."""
    _kind = "blanker"

    def __init__(self, rx, block: int, guard: int, ramp: int, beta: float = 0.25, cap: float = 2.0, device: int = 0):
        rx = [tuple(r) for r in rx]
        self.nrx, self.device = len(rx), device
        arr = (BlankerRx * max(self.nrx, 1))()
        for j, (thr, flags) in enumerate(rx):
            arr[j] = BlankerRx(float(thr), int(flags) & 0xFFFFFFFF)
        self.block, self.guard, self.ramp, self.beta, self.cap = int(block), int(guard), int(ramp), float(beta), float(cap)
        self.params = BlankerParams(_clip(block), _clip(guard), _clip(ramp), beta, cap)
        h = C.c_void_p()
        check(ddc_lib().pddc_blanker_create(C.byref(h), device, self.nrx, C.byref(self.params), arr))
        self._h = h
        self.delay = int(ddc_lib().pddc_blanker_delay(h))

    def process(self, z, out=None, stream=None):
        """One batch: z a complex64 CUDA tensor [nrx, n] whose rows are contiguous (any row stride: the view
        Tuner.process returns is fine).  -> complex64 [nrx, n] (a view of `out`, a complex64 CUDA tensor [nrx, capacity]
        with contiguous rows, if given): output i is input i - delay of the stream.  `out` must not overlap z."""
        import torch
        if not self._rows(z, torch.complex64):
            raise PddcError(-1, "blanker: z must be a complex64 tensor [nrx, n] with contiguous rows")
        n = int(z.shape[1])
        out, cap = self._out(out, n, torch.complex64, "out must be a complex64")
        check(ddc_lib().pddc_blanker_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)),
                                             out.data_ptr() if out.numel() else None, cap, self._stream(stream)))
        return out[:, :n]

    def set_rx(self, rx: int, thr: float, flags: int = 0):
        """receiver rx from the next input sample on; nothing carried is reset"""
        check(ddc_lib().pddc_blanker_set_rx(self._h, int(rx), float(thr), int(flags) & 0xFFFFFFFF))

    def read(self, stream=None):
        """-> numpy structured array [nrx] (ref, triggers, blanked) after the batches submitted so far (it waits for
        them)"""
        import numpy as np
        st = np.zeros(self.nrx, dtype=blanker_status_dtype())
        check(ddc_lib().pddc_blanker_read(self._h, st.ctypes.data, self._stream(stream)))
        return st


PDDC_WB_ON = 0x1


def wblank_tile_samples() -> int:
    """pddc_wblank_tile_samples: samples per tile of the gate kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_wblank_tile_samples())


def wblank_run_samples() -> int:
    """pddc_wblank_run_samples: samples one workgroup walks under the current "wblank_run" tunable (one tile when it is
    automatic); host arithmetic, no device"""
    return int(ddc_lib().pddc_wblank_run_samples())


def wblank_status_dtype():
    """pddc_wblank_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("mean", np.uint64), ("triggers", np.uint64), ("blanked", np.uint64), ("samples", np.uint64)])


def _wblank_thr16(thr) -> int:
    """a power ratio as the C ABI takes it: sixteenths, rounded; out of range stays out of range"""
    t = float(thr) * 16.0
    return int(round(t)) if 0.0 <= t < 4.0e9 else 0xFFFFFFFF


class WBlank(_StreamObject):
    """pddc_wblank: the wideband blanker -- impulse blanking on the packed 24-bit ADC stream itself, in front of Pipeline,
    Bank, Spectrum and Channelizer, which take its output as they take the stream (include/perseus_ddc.h).  Integers
    only: the power sums of every `block` samples (a power of two 64 .. 4096) are metered, the reference is the least of
    the last `history` (1 .. 16) block means, a sample whose power exceeds the reference times `thr` (1 .. 4096, in
    sixteenths) is a trigger; the output is the input delayed by `delay` = guard + 2^ramp_log2 - 1 samples, zero within
    `guard` samples of a trigger and scaled by 1 / 2^ramp_log2 .. (2^ramp_log2 - 1) / 2^ramp_log2 on the ramps beside it;
    every other sample keeps its six bytes.  Feed it every batch in order on one stream; all bytes and counters are the
    same however the stream is cut (on multiples of 8 samples).  The last `delay` inputs come out when `delay` more
    samples are fed."""
    _kind = "wblank"

    def __init__(self, block: int, history: int, guard: int, ramp_log2: int, thr: float = 16.0, on: bool = True,
                 device: int = 0):
        self.device = device
        self.block, self.history, self.guard, self.ramp_log2 = int(block), int(history), int(guard), int(ramp_log2)
        self.params = WBlankParams(_clip(block), _clip(history), _clip(guard), _clip(ramp_log2))
        h = C.c_void_p()
        check(ddc_lib().pddc_wblank_create(C.byref(h), device, C.byref(self.params), _wblank_thr16(thr),
                                           PDDC_WB_ON if on else 0))
        self._h = h
        self.delay = int(ddc_lib().pddc_wblank_delay(h))

    def process(self, packed, nsamples=None, out=None, stream=None):
        """One batch: a torch uint8 CUDA tensor of packed samples (or a device address with nsamples).  -> uint8 tensor
        of 6 nsamples bytes (the front of `out`, a contiguous uint8 CUDA tensor that does not overlap the input, if
        given): sample i of it is input i - delay of the stream."""
        import torch
        ptr, nsamples = _packed_arg(self._kind, packed, nsamples)
        nsamples = int(nsamples)
        if out is None:
            out = torch.empty(6 * max(nsamples, 0), dtype=torch.uint8, device=torch.device("cuda", self.device))
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < 6 * nsamples:
            raise PddcError(-1, "wblank: out must be a contiguous uint8 tensor of at least 6 nsamples bytes")
        check(ddc_lib().pddc_wblank_process(self._h, ptr if nsamples else None, nsamples,
                                            out.data_ptr() if nsamples else None, self._stream(stream)))
        return out.view(-1)[:6 * nsamples]

    def set(self, thr: float, on: bool = True):
        """threshold and ON / OFF from the next input sample on; nothing carried is reset"""
        check(ddc_lib().pddc_wblank_set(self._h, _wblank_thr16(thr), PDDC_WB_ON if on else 0))

    def read(self, stream=None):
        """-> numpy structured scalar (mean, triggers, blanked, samples) after the batches submitted so far (it waits for
        them)"""
        import numpy as np
        st = np.zeros(1, dtype=wblank_status_dtype())
        check(ddc_lib().pddc_wblank_read(self._h, st.ctypes.data, self._stream(stream)))
        return st[0]


PDDC_SCOPE_CENTERED = 0x1


def scope_lines(nfft: int, hop: int, avg: int, samples_before: int, n: int) -> int:
    """pddc_scope_lines: lines per slot that n samples after samples_before complete; host arithmetic, no device"""
    return int(ddc_lib().pddc_scope_lines(nfft, hop, avg, samples_before, n))


def scope_block_items(nfft: int) -> int:
    """pddc_scope_block_items: (slot, line) items one block of the kernel takes side by side; host arithmetic, no device"""
    return int(ddc_lib().pddc_scope_block_items(nfft))


def scope_db(lines, avg: int, window):
    """10 log10(P / (avg (sum w)^2)): a full-scale complex tone on a bin centre reads 0 dB.  `lines` a torch tensor or an
    array (what Scope.process returns), `window` the window the scope was made with.  -> numpy float64, same shape."""
    import numpy as np
    p = lines.detach().cpu().numpy() if hasattr(lines, "detach") else np.asarray(lines)
    w = np.asarray(window, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(p.astype(np.float64) / (float(avg) * w.sum() ** 2))


class Scope(_StreamObject):
    """pddc_scope: the receivers' own spectrum and waterfall lines, on the device (include/perseus_ddc.h).  It reads the
    complex64 rows that Tuner, Blanker or RxFilter return, in place, and writes per display slot the power spectrum of
    windowed segments of nfft (256 .. 4096) samples, `hop` (nfft/16 .. nfft, default nfft/2) apart, summed over `avg`
    segments per line.  rows: per slot the watched row of z (several slots may watch one row), or -1 for off; window
    float32[nfft] (default: periodic Hann); centered: position k holds bin (k + nfft/2) mod nfft.  Feed it every batch
    in order on one stream; all lines are bit-identical however the series is cut."""
    _kind = "scope"

    def __init__(self, nsrc: int, rows, nfft: int, hop=None, avg: int = 1, window=None, centered: bool = False,
                 device: int = 0):
        import numpy as np
        self.nsrc, self.device, self.nfft, self.avg = int(nsrc), device, int(nfft), int(avg)
        self.hop = int(self.nfft // 2 if hop is None else hop)
        self.centered = bool(centered)
        if window is None:
            if self.nfft <= 0:
                raise PddcError(-1, "scope: nfft must be positive")
            window = hann_window(self.nfft)
        w = np.ascontiguousarray(np.asarray(window, dtype=np.float32).reshape(-1))
        if w.size != self.nfft:
            raise PddcError(-1, f"scope: window of {w.size} values for nfft {self.nfft}")
        self.window = w
        r = np.ascontiguousarray(np.clip(np.asarray(rows, dtype=np.int64).reshape(-1), -2, 1 << 30), dtype=np.int32)
        self.nslots = self.nrx = int(r.size)
        h = C.c_void_p()
        check(ddc_lib().pddc_scope_create(C.byref(h), device, _clip(nsrc), self.nslots, r.ctypes.data_as(C.POINTER(C.c_int)),
                                          _clip(nfft), _clip(self.hop), _clip(avg), w.ctypes.data_as(C.POINTER(C.c_float)),
                                          PDDC_SCOPE_CENTERED if centered else 0))
        self._h = h

    def next_lines(self, n: int) -> int:
        """lines per slot the next process() of n samples writes (known from sizes alone)"""
        return int(ddc_lib().pddc_scope_next_lines(self._h, n))

    def process(self, z, out=None, stream=None):
        """One batch: z a complex64 CUDA tensor [nsrc, n] whose rows are contiguous (any row stride: the views Tuner,
        Blanker and RxFilter return are fine).  -> float32 [nslots, lines, nfft], the lines this batch completed (a view
        of `out`, a contiguous float32 CUDA tensor [nslots, capacity, nfft], if given)."""
        import torch
        if not (z.dtype == torch.complex64 and z.dim() == 2 and z.shape[0] == self.nsrc and (z.shape[1] <= 1 or z.stride(1) == 1)):
            raise PddcError(-1, "scope: z must be a complex64 tensor [nsrc, n] with contiguous rows")
        n = int(z.shape[1])
        due = self.next_lines(n)
        if out is None:
            out = torch.empty((self.nslots, due, self.nfft), dtype=torch.float32, device=torch.device("cuda", self.device))
        elif not (out.dtype == torch.float32 and out.dim() == 3 and out.shape[0] == self.nslots and out.shape[2] == self.nfft
                  and out.is_contiguous()):
            raise PddcError(-1, "scope: out must be a contiguous float32 tensor [nslots, capacity, nfft]")
        c = C.c_size_t()
        check(ddc_lib().pddc_scope_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)) if n else 0,
                                           out.data_ptr() if out.numel() else None, int(out.shape[1]), C.byref(c),
                                           self._stream(stream)))
        return out[:, :c.value]

    def set_slot(self, slot: int, row: int):
        """slot watches `row` (-1: off) from the next batch on; a new row starts from zeros, the same row changes nothing"""
        check(ddc_lib().pddc_scope_set_slot(self._h, _clip(slot), max(-2, min(int(row), 1 << 30))))


AUDIO_MAX_RATIO, AUDIO_MAX_DECIM = 1 << 24, 16


def audio_outputs(L: int, M: int, inputs_before: int, n: int) -> int:
    """pddc_audio_outputs: outputs of n inputs after inputs_before, ceil((before + n) L / M) - ceil(before L / M); host
    arithmetic, no device"""
    return int(ddc_lib().pddc_audio_outputs(L, M, inputs_before, n))


def audio_ratio(fs_hz, hop: int, decim: int, out_rate):
    """The ratio that takes the chain's rate fs_hz / (hop * decim) -- Channelizer hop, Tuner decim -- to out_rate,
    reduced, in exact rational arithmetic: audio_ratio(80e6, 512, 16, 48000) is (3072, 625).  Raises when L or M exceeds
    2^24 or M > 16 L (Audio's limits).  -> (L, M)"""
    from fractions import Fraction
    f = Fraction(out_rate) * int(hop) * int(decim) / Fraction(fs_hz)
    if f <= 0:
        raise PddcError(-1, "audio_ratio: the rates, hop and decim must be positive")
    L, M = f.numerator, f.denominator
    if L > AUDIO_MAX_RATIO or M > AUDIO_MAX_RATIO or M > AUDIO_MAX_DECIM * L:
        raise PddcError(-1, f"audio_ratio: {L}/{M} is outside Audio's limits (1 .. 2^24 each, M <= 16 L)")
    return L, M


def audio_prototype(phases: int, taps: int, cutoff=None, beta: float = 9.0):
    """Audio's prototype: a Kaiser-windowed sinc over phases * taps points, -6 dB at `cutoff` cycles per INPUT sample
    (default 0.45; for a ratio L/M below 1 pass 0.45 * L / M, so that the band ends below the output's Nyquist
    frequency), double, normalised so that the sum is `phases` (every phase then sums to about 1), rounded once.
    -> numpy float32[phases * taps]."""
    import numpy as np
    P, T = int(phases), int(taps)
    if P <= 0 or T <= 0:
        raise PddcError(-1, "audio_prototype: phases and taps must be positive")
    fc = 0.45 if cutoff is None else float(cutoff)
    t = (np.arange(P * T, dtype=np.float64) - (P * T - 1) / 2.0) / P     # in input samples
    g = np.sinc(2.0 * fc * t) * np.kaiser(P * T, float(beta))
    return (g * (P / g.sum())).astype(np.float32)


class Audio(_StreamObject):
    """pddc_audio: the receivers' real float32 series, such as Demod.process returns, resampled by the exact ratio L/M
    (audio_ratio) with an interpolated polyphase filter -- `phases` stored phases of `taps` taps, the prototype `proto`
    (audio_prototype; default: one for this ratio), linear interpolation between neighbouring phases -- as float32 and /
    or saturated int16 PCM, p = clamp(rint(y * scale)), on the device (include/perseus_ddc.h).  Feed it every batch in
    order on one stream; outputs are bit-identical however the series is cut."""
    _kind = "audio"

    def __init__(self, nrx: int, L: int, M: int, phases: int = 128, taps: int = 32, proto=None, scale: float = 32767.0,
                 device: int = 0):
        import math
        import numpy as np
        L, M = int(L), int(M)
        if not (0 < L < 1 << 32 and 0 < M < 1 << 32):
            raise PddcError(-1, "audio: L and M must be in 1 .. 2^24")
        if proto is None:
            proto = audio_prototype(phases, taps, 0.45 * min(1.0, L / M))
        g = np.ascontiguousarray(np.asarray(proto, dtype=np.float32).reshape(-1))
        if g.size != int(phases) * int(taps):
            raise PddcError(-1, "audio: the prototype must have phases * taps values")
        d = math.gcd(L, M)
        self.nrx, self.device, self.L, self.M = int(nrx), device, L // d, M // d
        self.phases, self.taps, self.proto, self.scale = int(phases), int(taps), g, float(scale)
        h = C.c_void_p()
        check(ddc_lib().pddc_audio_create(C.byref(h), device, self.nrx, L, M, self.phases, self.taps,
                                          g.ctypes.data_as(C.POINTER(C.c_float)), self.scale))
        self._h = h

    def next_outputs(self, n: int) -> int:
        """outputs per receiver the next process() of n inputs writes (known from sizes alone)"""
        c = C.c_size_t()
        check(ddc_lib().pddc_audio_next_outputs(self._h, n, C.byref(c)))
        return int(c.value)

    def process(self, x, f32: bool = True, i16: bool = False, out_f32=None, out_i16=None, stream=None):
        """One batch: a float32 CUDA tensor [nrx, n] whose rows are contiguous (any row stride: the view Demod.process
        returns is fine).  -> float32 [nrx, count] if f32, int16 [nrx, count] if i16, both as a tuple if both (views of
        `out_f32` / `out_i16`, CUDA tensors [nrx, capacity] with contiguous rows, if given; giving one asks for it)."""
        import torch
        if not self._rows(x, torch.float32):
            raise PddcError(-1, "audio: x must be a float32 tensor [nrx, n] with contiguous rows")
        f32, i16 = f32 or out_f32 is not None, i16 or out_i16 is not None
        if not (f32 or i16):
            raise PddcError(-1, "audio: ask for float32, int16 or both")
        n = int(x.shape[1])
        due = self.next_outputs(n)
        outs, cap = [None, None], [0, 0]
        for i, (want, out, dt, what) in enumerate(((f32, out_f32, torch.float32, "out_f32 must be a torch.float32"),
                                                   (i16, out_i16, torch.int16, "out_i16 must be a torch.int16"))):
            if want:
                outs[i], cap[i] = self._out(out, due, dt, what)
        ptr = [o.data_ptr() if o is not None and o.numel() else None for o in outs]
        c = C.c_size_t()
        check(ddc_lib().pddc_audio_process(self._h, x.data_ptr() if n else None, n, int(x.stride(0)), ptr[0], cap[0], ptr[1],
                                           cap[1], C.byref(c), self._stream(stream)))
        views = [o[:, :c.value] for o in outs if o is not None]
        return views[0] if len(views) == 1 else tuple(views)


PDDC_MIX_LIMIT = 0x1


def mixer_chunk() -> int:
    """pddc_mixer_chunk: C, the active receivers per chunk sum of the mixer's summation tree; host arithmetic, no device"""
    return int(ddc_lib().pddc_mixer_chunk())


def mixer_tile_outputs() -> int:
    """pddc_mixer_tile_outputs: samples per tile of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_mixer_tile_outputs())


def mixer_outputs(block: int, samples_before: int, n: int) -> int:
    """pddc_mixer_outputs: outputs per bus of the limiter for n samples after samples_before, block * (max(0, (before + n)
    // block - 1) - max(0, before // block - 1)); 0 for an unsupported block length; host arithmetic, no device"""
    block = int(block)
    return int(ddc_lib().pddc_mixer_outputs(block if -1 << 31 <= block < 1 << 31 else 0, samples_before, n))


def mixer_status_dtype():
    """pddc_mixer_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("peak", np.float32), ("gain", np.float32), ("min_gain", np.float32)])


def mixer_pan(gain_db: float, pan: float):
    """The constant-power stereo pair of a receiver at gain_db decibels and position pan, -1 (left) .. 0 (centre) .. +1
    (right): (g cos t, g sin t) with g = 10^(gain_db / 20) and t = (pan + 1) pi / 4, so left^2 + right^2 = g^2.
    -> (left, right) as float32 values"""
    import numpy as np
    if not -1.0 <= float(pan) <= 1.0:
        raise PddcError(-1, "mixer_pan: pan must be in -1 .. 1")
    g, t = 10.0 ** (float(gain_db) / 20.0), (float(pan) + 1.0) * math.pi / 4.0
    return float(np.float32(g * math.cos(t))), float(np.float32(g * math.sin(t)))


class Mixer(_StreamObject):
    """pddc_mixer: the receivers' real float32 series, such as Audio, Squelch and Adapt write, summed into Q output buses
    on the device (include/perseus_ddc.h).  gains: [nrx][Q] target gains (1 <= Q <= 8; mixer_pan gives a stereo pair); a
    change (set_rx) is ramped linearly over `ramp` samples from the next batch on; a receiver whose gains are all zero and
    whose ramp has ended is silent: not read, not in the sum.  limit = (block, ceil, rel) puts a peak limiter on every
    bus: the gain follows the block peaks one block ahead (the outputs come one block late), falls at once, recovers by
    `rel` per block, and |out| <= ceil exactly.  Outputs: planar float32 [Q, count] and / or interleaved int16 frames
    [count, Q], p = clamp(rint(out * scale)).  The sum is a fixed tree over the active receivers: feed it every batch in
    order on one stream; outputs are bit-identical however the series is cut."""
    _kind = "mixer"

    def __init__(self, gains, ramp: int, limit=None, scale: float = 32767.0, device: int = 0):
        import numpy as np
        g = np.ascontiguousarray(np.asarray(gains, dtype=np.float32))
        if g.ndim != 2:
            raise PddcError(-1, "mixer: gains must be [nrx][nbus]")
        self.nrx, self.nbus, self.device = int(g.shape[0]), int(g.shape[1]), device
        self.ramp, self.limit, self.scale = int(ramp), None if limit is None else tuple(limit), float(scale)
        block, ceil, rel = self.limit if self.limit else (0, 0.0, 0.0)
        self.block = int(block)
        self.params = MixerParams(_clip(self.nbus), _clip(ramp), PDDC_MIX_LIMIT if self.limit else 0, _clip(block), ceil, rel,
                                  self.scale)
        h = C.c_void_p()
        check(ddc_lib().pddc_mixer_create(C.byref(h), device, self.nrx, C.byref(self.params),
                                          g.ctypes.data_as(C.POINTER(C.c_float)) if g.size else None))
        self._h = h

    def next_outputs(self, n: int) -> int:
        """outputs per bus the next process() of n samples writes (known from sizes alone)"""
        c = C.c_size_t()
        check(ddc_lib().pddc_mixer_next_outputs(self._h, n, C.byref(c)))
        return int(c.value)

    def process(self, a, f32: bool = True, i16: bool = False, out_f32=None, out_i16=None, stream=None):
        """One batch: a float32 CUDA tensor [nrx, n] whose rows are contiguous (any row stride: the view Audio.process
        returns is fine).  -> float32 [Q, count] if f32, int16 [count, Q] if i16, both as a tuple if both (views of
        `out_f32`, a CUDA tensor [Q, capacity] with contiguous rows, and `out_i16`, a contiguous CUDA tensor [capacity,
        Q], if given; giving one asks for it).  No output may overlap a."""
        import torch
        if not self._rows(a, torch.float32):
            raise PddcError(-1, "mixer: a must be a float32 tensor [nrx, n] with contiguous rows")
        f32, i16 = f32 or out_f32 is not None, i16 or out_i16 is not None
        if not (f32 or i16):
            raise PddcError(-1, "mixer: ask for float32, int16 or both")
        n, Q = int(a.shape[1]), self.nbus
        due = self.next_outputs(n)
        dev = torch.device("cuda", self.device)
        fcap = icap = 0
        if f32:
            if out_f32 is None:
                out_f32 = torch.empty((Q, due), dtype=torch.float32, device=dev)
            elif not (out_f32.dtype == torch.float32 and out_f32.dim() == 2 and out_f32.shape[0] == Q
                      and (out_f32.shape[1] <= 1 or out_f32.stride(1) == 1)):
                raise PddcError(-1, "mixer: out_f32 must be a float32 tensor [nbus, capacity] with contiguous rows")
            fcap = int(out_f32.stride(0)) if out_f32.shape[1] >= due else int(out_f32.shape[1])
        if i16:
            if out_i16 is None:
                out_i16 = torch.empty((due, Q), dtype=torch.int16, device=dev)
            elif not (out_i16.dtype == torch.int16 and out_i16.dim() == 2 and out_i16.shape[1] == Q and out_i16.is_contiguous()):
                raise PddcError(-1, "mixer: out_i16 must be a contiguous int16 tensor [capacity, nbus]")
            icap = int(out_i16.shape[0])
        ptr = [o.data_ptr() if o is not None and o.numel() else None for o in (out_f32, out_i16)]
        c = C.c_size_t()
        check(ddc_lib().pddc_mixer_process(self._h, a.data_ptr() if n else None, n, int(a.stride(0)), ptr[0], fcap, ptr[1], icap,
                                           C.byref(c), self._stream(stream)))
        views = ([out_f32[:, :c.value]] if f32 else []) + ([out_i16[:c.value]] if i16 else [])
        return views[0] if len(views) == 1 else tuple(views)

    def set_rx(self, rx: int, gains):
        """receiver rx: new target gains [Q], reached over `ramp` samples from the first sample of the next batch on,
        starting at the gain of the last sample processed; two calls before one batch count as one"""
        import numpy as np
        g = np.ascontiguousarray(np.asarray(gains, dtype=np.float32).reshape(-1))
        if g.size != self.nbus:
            raise PddcError(-1, "mixer: set_rx takes one gain per bus")
        check(ddc_lib().pddc_mixer_set_rx(self._h, int(rx), g.ctypes.data_as(C.POINTER(C.c_float))))

    def read(self, clear: bool = False, stream=None):
        """-> numpy structured array [Q] (peak, gain, min_gain) after the batches submitted so far (it waits for them);
        clear: peak restarts at 0 and min_gain at 1 for the samples after the call"""
        import numpy as np
        st = np.zeros(self.nbus, dtype=mixer_status_dtype())
        check(ddc_lib().pddc_mixer_read(self._h, st.ctypes.data, 1 if clear else 0, self._stream(stream)))
        return st


class _Decoder(_StreamObject):
    """What Fsk, Morse, Psk, Sitor, Fax and Mfsk share: the capacity bound, the chars and counts outputs of process() and the status read
    (Fax's records are its lines, Mfsk's its symbols: `_bound` names the bound's function)."""
    _bound = "max_chars"

    def max_chars(self, n: int) -> int:
        """pddc_<kind>_max_chars: the most characters one receiver can end in a batch of n samples (host arithmetic)"""
        c = C.c_size_t()
        check(getattr(ddc_lib(), f"pddc_{self._kind}_{self._bound}")(self._h, int(n), C.byref(c)))
        return int(c.value)

    def _batch(self, z, chars, counts):
        """What process() begins with: z tested, chars and counts tested or made.  -> (n, chars, counts, the capacity of
        chars for the C ABI).  The ABI takes the row stride in characters; a capacity below the bound must reach it as
        one (PDDC_ECAPACITY)."""
        import torch
        if not self._rows(z, torch.complex64):
            raise PddcError(-1, f"{self._kind}: z must be a complex64 tensor [nrx, n] with contiguous rows")
        n = int(z.shape[1])
        bound = self.max_chars(n)
        if chars is None:
            chars = torch.empty((self.nrx, max(bound, 1), 4), dtype=torch.int32, device=torch.device("cuda", self.device))
        elif not (chars.dtype == torch.int32 and chars.dim() == 3 and chars.shape[0] == self.nrx and chars.shape[2] == 4
                  and chars[0].is_contiguous()):
            raise PddcError(-1, f"{self._kind}: chars must be an int32 tensor [nrx, capacity, 4] with contiguous rows")
        if counts is None:
            counts = torch.empty((self.nrx,), dtype=torch.int32, device=torch.device("cuda", self.device))
        elif not (counts.dtype == torch.int32 and counts.dim() == 1 and counts.shape[0] == self.nrx and counts.is_contiguous()):
            raise PddcError(-1, f"{self._kind}: counts must be a contiguous int32 tensor [nrx]")
        return n, chars, counts, int(chars.stride(0)) // 4 if chars.shape[1] >= bound else int(chars.shape[1])

    def _read(self, dtype, stream):
        """read(): -> numpy structured array [nrx] of `dtype`, the pddc_<kind>_status records"""
        import numpy as np
        st = np.zeros(self.nrx, dtype=dtype)
        check(getattr(ddc_lib(), f"pddc_{self._kind}_read")(self._h, st.ctypes.data, self._stream(stream)))
        return st


PDDC_FSK_ON, PDDC_FSK_REVERSE, PDDC_FSK_RESTART = 0x1, 0x2, 0x4
PDDC_FSK_FRAMING = 0x1
PDDC_FSK_IDLE, PDDC_FSK_START, PDDC_FSK_DATA, PDDC_FSK_STOP = 0, 1, 2, 3


def fsk_tile_outputs() -> int:
    """pddc_fsk_tile_outputs: samples per tile of the kernel's walk; host arithmetic, no device"""
    return int(ddc_lib().pddc_fsk_tile_outputs())


def fsk_char_dtype():
    """pddc_fsk_char as a numpy structured dtype (16 bytes)"""
    import numpy as np
    return np.dtype([("start", np.uint64), ("code", np.uint16), ("flags", np.uint16), ("quality", np.float32)])


def fsk_status_dtype():
    """pddc_fsk_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("chars", np.uint32), ("framing", np.uint32), ("false_starts", np.uint32), ("state", np.uint32),
                     ("d_last", np.float32)])


def fsk_modem(rate_hz: float, baud: float, mark_hz: float, space_hz: float, W: int, nbits: int = 5):
    """A modem for Fsk's bank: the two matched filters h[t] = w[t] exp(+2 pi i f t / rate_hz), f = mark_hz and space_hz
    (offsets from the receiver's tuned frequency, either sign), w a boxcar over min(W, round(rate_hz / baud)) samples
    with sum 1 and zero beyond, computed in double and rounded once; inc = round(2^32 baud / rate_hz).
    -> (hm complex64[W], hs complex64[W], inc, nbits)"""
    import numpy as np
    W, rate, baud = int(W), float(rate_hz), float(baud)
    if W <= 0 or not rate > 0.0 or not baud > 0.0:
        raise PddcError(-1, "fsk_modem: W, the rate and the baud rate must be positive")
    L = min(W, max(1, int(round(rate / baud))))
    t = np.arange(W, dtype=np.float64)
    w = np.where(t < L, 1.0 / L, 0.0)
    hm, hs = ((w * np.exp(2j * np.pi * float(f) * t / rate)).astype(np.complex64) for f in (mark_hz, space_hz))
    return hm, hs, int(round(4294967296.0 * baud / rate)), int(nbits)


_ITA2_LTRS = "\x00E\nA SIU\rDRJNFCKTZLWHYPQOBG\x0eMXV\x0f"
_ITA2_FIGS = "\x003\n- '87\r\x054\x07,!:(5+)2#6019?&\x0e./=\x0f"


def fsk_ita2(codes, flags=None) -> str:
    """The text of 5-bit ITA2 codes (pddc_fsk_char.code: the first data bit in bit 0, mark = 1), host only: letters
    and figures with the two shift codes (27 figures, 31 letters; they give no character themselves, and the text
    starts in letters).  A character whose flags hold PDDC_FSK_FRAMING, and a code above 31, becomes U+FFFD."""
    out, table = [], _ITA2_LTRS
    for i, c in enumerate(codes):
        c = int(c)
        if (flags is not None and int(flags[i]) & PDDC_FSK_FRAMING) or not 0 <= c < 32:
            out.append("\ufffd")
        elif c == 27:
            table = _ITA2_FIGS
        elif c == 31:
            table = _ITA2_LTRS
        else:
            out.append(table[c])
    return "".join(out)


class Fsk(_Decoder):
    """pddc_fsk: start-stop FSK (RTTY) decoding of every receiver's complex series, such as Tuner, Blanker, RxFilter or
    Carrier write, on the device (include/perseus_ddc.h): two matched filters of W complex taps and a start-stop
    receiver per receiver; the output is characters, not samples.  bank: up to 16 modems (hm, hs, inc, nbits), as
    fsk_modem gives them, every hm and hs of W taps; sel: one (modem, flags) per receiver, flags PDDC_FSK_ON |
    PDDC_FSK_REVERSE.  Feed it every batch in order on one stream; every output bit is the same however the series is
    cut."""
    _kind = "fsk"

    def __init__(self, bank, sel, W: int, device: int = 0):
        import numpy as np
        bank = [tuple(b) for b in bank]
        sel = [tuple(r) for r in sel]
        self.W, self.nrx, self.nmodems, self.device = int(W), len(sel), len(bank), device
        taps = np.zeros((max(self.nmodems, 1), 2, max(self.W, 1)), np.complex64)
        for b, (hm, hs, _, _) in enumerate(bank):
            for i, h in enumerate((hm, hs)):
                h = np.asarray(h, dtype=np.complex64).reshape(-1)
                if h.size != self.W:
                    raise PddcError(-1, f"fsk: modem {b}: {h.size} taps for a window of {self.W}")
                taps[b, i] = h
        inc = np.array([max(0, min(int(b[2]), (1 << 32) - 1)) for b in bank] or [0], dtype=np.uint32)
        nbits = np.array([_clip(b[3]) for b in bank] or [0], dtype=np.int32)
        arr = (FskRx * max(self.nrx, 1))()
        for j, (modem, flags) in enumerate(sel):
            arr[j] = FskRx(_clip(modem), int(flags) & 0xFFFFFFFF)
        h = C.c_void_p()
        check(ddc_lib().pddc_fsk_create(C.byref(h), device, self.nrx, _clip(W), self.nmodems,
                                        taps.ctypes.data_as(C.POINTER(C.c_float)), inc.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        nbits.ctypes.data_as(C.POINTER(C.c_int)), arr))
        self._h = h

    def process(self, z, chars=None, counts=None, d=None, want_d: bool = False, stream=None):
        """One batch: a complex64 CUDA tensor [nrx, n] whose rows are contiguous (any row stride).  -> (chars, counts) or,
        with want_d or d given, (chars, counts, d): chars int32 [nrx, capacity, 4], four words per pddc_fsk_char
        (`.cpu().numpy().view(fsk_char_dtype())[..., 0]` gives the records), of which the first counts[j] (int32 [nrx])
        of row j are written; d float32 [nrx, n], the soft discriminator.  chars, counts and d, if given, are
        tensors of these kinds (chars and d with any capacity that suffices); no output may overlap z."""
        n, chars, counts, ccap = self._batch(z, chars, counts)
        dcap = 0
        if d is not None or want_d:
            import torch
            d, dcap = self._out(d, n, torch.float32, "d must be a float32")
        check(ddc_lib().pddc_fsk_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)),
                                         chars.data_ptr() if chars.numel() else None, ccap, counts.data_ptr(),
                                         d.data_ptr() if d is not None and d.numel() else None, dcap, self._stream(stream)))
        return (chars, counts) if d is None else (chars, counts, d[:, :n])

    def set_rx(self, rx: int, modem: int, flags: int):
        """receiver rx from the next batch's first sample on: PDDC_FSK_RESTART, or OFF -> ON, starts it afresh (the
        counters stay); another modem keeps the carried inputs and drops a character in progress"""
        check(ddc_lib().pddc_fsk_set_rx(self._h, int(rx), _clip(modem), int(flags) & 0xFFFFFFFF))

    def read(self, stream=None):
        """-> numpy structured array [nrx] (chars, framing, false_starts, state, d_last) after the batches submitted so
        far (it waits for them)"""
        return self._read(fsk_status_dtype(), stream)


PDDC_MORSE_ON, PDDC_MORSE_FIXED, PDDC_MORSE_RESTART = 0x1, 0x2, 0x4
PDDC_MORSE_WORD, PDDC_MORSE_LONG = 0x1, 0x2


def morse_tile_outputs() -> int:
    """pddc_morse_tile_outputs: samples per tile of the kernel's walk (tiles are aligned to the object's sample count);
    host arithmetic, no device"""
    return int(ddc_lib().pddc_morse_tile_outputs())


def morse_char_dtype():
    """pddc_morse_char as a numpy structured dtype (16 bytes)"""
    import numpy as np
    return np.dtype([("start", np.uint64), ("code", np.uint16), ("nel", np.uint8), ("flags", np.uint8), ("two", np.uint32)])


def morse_status_dtype():
    """pddc_morse_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("chars", np.uint32), ("marks", np.uint32), ("two", np.uint32), ("nel", np.uint32), ("key", np.uint32),
                     ("pk", np.float32), ("fl", np.float32)])


def morse_keyer(rate_hz: float, wpm: float, W: int, wpm_min: float = 5, wpm_max: float = 60, shift: int = 2):
    """A keyer for Morse's bank.  A dot lasts 1.2 / wpm seconds (PARIS), so two dots are 2.4 rate_hz / wpm samples: two0 at
    wpm, two_min at wpm_max and two_max at wpm_min, each round(256 x that) and brought into 512 .. 2^28 with two_min <=
    two0 <= two_max.  The taps are a Hann window over L = min(W, max(1, round(0.6 rate_hz / wpm))) samples, about half
    a dot at wpm, w[t] = 1 - cos(2 pi (t + 1) / (L + 1)), of unit sum, computed in double and rounded once, zero
    beyond.  -> (h float32[W], two0, two_min, two_max, shift)"""
    import numpy as np
    W, rate, wpm = int(W), float(rate_hz), float(wpm)
    if W <= 0 or not rate > 0.0 or not wpm > 0.0 or not 0.0 < float(wpm_min) <= float(wpm_max):
        raise PddcError(-1, "morse_keyer: W, the rate and the speeds must be positive, wpm_min <= wpm_max")
    L = min(W, max(1, int(round(0.6 * rate / wpm))))
    t = np.arange(W, dtype=np.float64)
    w = np.where(t < L, 1.0 - np.cos(2.0 * np.pi * (t + 1.0) / (L + 1.0)), 0.0)
    two = [min(max(int(round(256.0 * 2.4 * rate / float(v))), 512), 1 << 28) for v in (wpm, wpm_max, wpm_min)]
    return (w / w.sum()).astype(np.float32), min(max(two[0], two[1]), two[2]), two[1], two[2], int(shift)


_MORSE_ITU = {".-": "A", "-...": "B", "-.-.": "C", "-..": "D", ".": "E", "..-.": "F", "--.": "G", "....": "H", "..": "I",
              ".---": "J", "-.-": "K", ".-..": "L", "--": "M", "-.": "N", "---": "O", ".--.": "P", "--.-": "Q", ".-.": "R",
              "...": "S", "-": "T", "..-": "U", "...-": "V", ".--": "W", "-..-": "X", "-.--": "Y", "--..": "Z",
              "-----": "0", ".----": "1", "..---": "2", "...--": "3", "....-": "4", ".....": "5", "-....": "6", "--...": "7",
              "---..": "8", "----.": "9", ".-.-.-": ".", "--..--": ",", "---...": ":", "..--..": "?", ".----.": "'", "-....-": "-",
              "-..-.": "/", "-.--.": "(", "-.--.-": ")", ".-..-.": '"', "-...-": "=", ".-.-.": "+", ".--.-.": "@", "..-..": "\u00c9"}
_MORSE_CODES = {int("1" + k.replace(".", "0").replace("-", "1"), 2): v for k, v in _MORSE_ITU.items()}


def morse_text(records) -> str:
    """The text of pddc_morse_char records (a numpy array of morse_char_dtype, or any sequence of records with code and
    flags), host only: the ITU table (letters, figures, punctuation, accented E), `?` for a code it does not hold or a
    character with PDDC_MORSE_LONG, a space in front of every character with PDDC_MORSE_WORD but the first."""
    out = []
    for i, c in enumerate(records):
        flags = int(c["flags"])
        if flags & PDDC_MORSE_WORD and i:
            out.append(" ")
        out.append("?" if flags & PDDC_MORSE_LONG else _MORSE_CODES.get(int(c["code"]), "?"))
    return "".join(out)


class Morse(_Decoder):
    """pddc_morse: CW decoding of every receiver's complex series, such as Tuner, Blanker, RxFilter or Carrier write, on the
    device (include/perseus_ddc.h): a real envelope filter of W taps, a block meter that places two thresholds between
    floor and peak, and the element timing with a speed tracker per receiver; the output is characters, not samples.
    bank: up to 16 keyers (h, two0, two_min, two_max, shift), as morse_keyer gives them, every h of W taps; sel: one
    (keyer, flags) per receiver, flags PDDC_MORSE_ON | PDDC_MORSE_FIXED.  Feed it every batch in order on one stream;
    every output bit is the same however the series is cut."""
    _kind = "morse"

    def __init__(self, bank, sel, W: int, a_on: float = 0.5, a_off: float = 0.3, rel: float = 1.0 / 16, relf: float = 1.0 / 64,
                 ratio: float = 4.0, device: int = 0):
        import numpy as np
        bank = [tuple(b) for b in bank]
        sel = [tuple(r) for r in sel]
        self.W, self.nrx, self.nkeyers, self.device = int(W), len(sel), len(bank), device
        taps = np.zeros((max(self.nkeyers, 1), max(self.W, 1)), np.float32)
        keyers = (MorseKeyer * max(self.nkeyers, 1))()
        u32 = lambda v: max(0, min(int(v), (1 << 32) - 1))
        for b, (h, two0, two_min, two_max, shift) in enumerate(bank):
            h = np.asarray(h, dtype=np.float32).reshape(-1)
            if h.size != self.W:
                raise PddcError(-1, f"morse: keyer {b}: {h.size} taps for a window of {self.W}")
            taps[b] = h
            keyers[b] = MorseKeyer(u32(two0), u32(two_min), u32(two_max), u32(shift))
        arr = (MorseRx * max(self.nrx, 1))()
        for j, (keyer, flags) in enumerate(sel):
            arr[j] = MorseRx(_clip(keyer), int(flags) & 0xFFFFFFFF)
        par = MorseParams(a_on, a_off, rel, relf, ratio)
        h = C.c_void_p()
        check(ddc_lib().pddc_morse_create(C.byref(h), device, self.nrx, _clip(W), self.nkeyers,
                                          taps.ctypes.data_as(C.POINTER(C.c_float)), keyers, C.byref(par), arr))
        self._h = h

    def process(self, z, chars=None, counts=None, p=None, want_p: bool = False, stream=None):
        """One batch: a complex64 CUDA tensor [nrx, n] whose rows are contiguous (any row stride).  -> (chars, counts) or,
        with want_p or p given, (chars, counts, p): chars int32 [nrx, capacity, 4], four words per pddc_morse_char
        (`.cpu().numpy().view(morse_char_dtype())[..., 0]` gives the records), of which the first counts[j] (int32 [nrx])
        of row j are written; p float32 [nrx, n], the envelope power.  chars, counts and p, if given, are tensors of
        these kinds (chars and p with any capacity that suffices); no output may overlap z."""
        n, chars, counts, ccap = self._batch(z, chars, counts)
        pcap = 0
        if p is not None or want_p:
            import torch
            p, pcap = self._out(p, n, torch.float32, "p must be a float32")
        check(ddc_lib().pddc_morse_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)),
                                           chars.data_ptr() if chars.numel() else None, ccap, counts.data_ptr(),
                                           p.data_ptr() if p is not None and p.numel() else None, pcap, self._stream(stream)))
        return (chars, counts) if p is None else (chars, counts, p[:, :n])

    def set_rx(self, rx: int, keyer: int, flags: int):
        """receiver rx from the next batch's first sample on: PDDC_MORSE_RESTART, or OFF -> ON, starts it afresh (the
        counters stay); another keyer does the same but keeps the carried inputs"""
        check(ddc_lib().pddc_morse_set_rx(self._h, int(rx), _clip(keyer), int(flags) & 0xFFFFFFFF))

    def read(self, stream=None):
        """-> numpy structured array [nrx] (chars, marks, two, nel, key, pk, fl) after the batches submitted so far (it
        waits for them)"""
        return self._read(morse_status_dtype(), stream)


PDDC_PSK_ON, PDDC_PSK_RESTART = 0x1, 0x4
PDDC_PSK_LONG = 0x1


def psk_tile_outputs() -> int:
    """pddc_psk_tile_outputs: samples per tile of the kernel's walk (tiles begin at the batch's first sample); host
    arithmetic, no device"""
    return int(ddc_lib().pddc_psk_tile_outputs())


def psk_char_dtype():
    """pddc_psk_char as a numpy structured dtype (16 bytes)"""
    import numpy as np
    return np.dtype([("start", np.uint64), ("code", np.uint16), ("nbits", np.uint8), ("flags", np.uint8), ("quality", np.float32)])


def psk_status_dtype():
    """pddc_psk_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("chars", np.uint32), ("symbols", np.uint32), ("acc", np.uint32), ("reg", np.uint32),
                     ("d_last", np.float32), ("x_last", np.float32)])


def psk_modem(W: int, samples_per_symbol: float, step: int = None, q: int = None):
    """A modem for Psk's bank at samples_per_symbol = rate / baud (8 or more; 31.25 baud is PSK31).  The taps are the
    raised-cosine pulse a PSK31 sender keys with, over L = min(W, round(2 sps)) samples: w[t] = 1 + cos(pi (t - (L - 1) /
    2) / sps) inside, zero beyond, of unit sum, computed in double and rounded once: the matched filter, whose output
    peaks at the symbol's middle (L - 1) / 2 samples later.  inc = round(2^32 / sps), at most 2^29; q = round(sps / 4)
    in 1 .. 64 with 4 q inc <= 2^32; step defaults to inc / 4, a quarter of a sample per reversal.
    -> (h float32[W], inc, q, step)"""
    import numpy as np
    W, sps = int(W), float(samples_per_symbol)
    if W <= 0 or not sps >= 8.0 or not sps <= float(1 << 32):
        raise PddcError(-1, "psk_modem: W must be positive and a symbol 8 .. 2^32 samples")
    L = min(W, max(1, int(round(2.0 * sps))))
    t = np.arange(W, dtype=np.float64)
    w = np.where(t < L, 1.0 + np.cos(np.pi * (t - (L - 1) / 2.0) / sps), 0.0)
    inc = min(max(int(round(float(1 << 32) / sps)), 1), 1 << 29)
    if q is None:
        q = int(round(sps / 4.0))
    q = min(max(int(q), 1), 64)
    while q > 1 and 4 * q * inc > (1 << 32):
        q -= 1
    step = inc // 4 if step is None else int(step)
    return (w / w.sum()).astype(np.float32), inc, q, step


# G3PLX Varicode, as published with PSK31 (Peter Martinez, RadCom 1998 / ARRL): ASCII 0 .. 127
_PSK_VARICODE = (
    "1010101011 1011011011 1011101101 1101110111 1011101011 1101011111 1011101111 1011111101 1011111111 11101111 11101 "
    "1101101111 1011011101 11111 1101110101 1110101011 1011110111 1011110101 1110101101 1110101111 1101011011 1101101011 "
    "1101101101 1101010111 1101111011 1101111101 1110110111 1101010101 1101011101 1110111011 1011111011 1101111111 1 "
    "111111111 101011111 111110101 111011011 1011010101 1010111011 101111111 11111011 11110111 101101111 111011111 1110101 "
    "110101 1010111 110101111 10110111 10111101 11101101 11111111 101110111 101011011 101101011 110101101 110101011 "
    "110110111 11110101 110111101 111101101 1010101 111010111 1010101111 1010111101 1111101 11101011 10101101 10110101 "
    "1110111 11011011 11111101 101010101 1111111 111111101 101111101 11010111 10111011 11011101 10101011 11010101 "
    "111011101 10101111 1101111 1101101 101010111 110110101 101011101 101110101 101111011 1010101101 111110111 111101111 "
    "111111011 1010111111 101101101 1011011111 1011 1011111 101111 101101 11 111101 1011011 101011 1101 111101011 10111111 "
    "11011 111011 1111 111 111111 110111111 10101 10111 101 110111 1111011 1101011 11011111 1011101 111010101 1010110111 "
    "110111011 1010110101 1011010111 1110110101").split()
_PSK_CODES = {int(b, 2): chr(i) for i, b in enumerate(_PSK_VARICODE)}


def psk_varicode(codes) -> str:
    """The text of Varicode codes (the `code` field of pddc_psk_char records, or any sequence of integers), host only:
    the G3PLX table of ASCII 0 .. 127 (space is 1, e is 11, t is 101, o is 111), U+FFFD for a code it does not hold."""
    return "".join(_PSK_CODES.get(int(c), "\ufffd") for c in codes)


def psk_varicode_bits(text: str):
    """The bits that send `text` (ASCII) in Varicode, each character followed by 00: a list of 0 / 1, a 0 being a
    phase reversal on the air.  Host only; what tests and tools key their signals with."""
    out = []
    for ch in text:
        out += [int(b) for b in _PSK_VARICODE[ord(ch)]] + [0, 0]
    return out


class Psk(_Decoder):
    """pddc_psk: differential BPSK (PSK31 and its faster siblings) decoding of every receiver's complex series, such as
    Tuner, Blanker, RxFilter or Carrier write, on the device (include/perseus_ddc.h): a real matched filter of W taps, a
    symbol clock that the envelope corrects at every phase reversal, the differential decision and the Varicode framing
    per receiver; the output is characters, not samples.
    bank: up to 16 modems (h, inc, q, step), as psk_modem gives them, every h of W taps; sel: one (modem, flags) per
    receiver, flags PDDC_PSK_ON.  Feed it every batch in order on one stream; every output bit is the same however the
    series is cut."""
    _kind = "psk"

    def __init__(self, bank, sel, W: int, device: int = 0):
        import numpy as np
        bank = [tuple(b) for b in bank]
        sel = [tuple(r) for r in sel]
        self.W, self.nrx, self.nmodems, self.device = int(W), len(sel), len(bank), device
        taps = np.zeros((max(self.nmodems, 1), max(self.W, 1)), np.float32)
        modems = (PskModem * max(self.nmodems, 1))()
        u32 = lambda v: max(0, min(int(v), (1 << 32) - 1))
        for b, (h, inc, q, step) in enumerate(bank):
            h = np.asarray(h, dtype=np.float32).reshape(-1)
            if h.size != self.W:
                raise PddcError(-1, f"psk: modem {b}: {h.size} taps for a window of {self.W}")
            taps[b] = h
            modems[b] = PskModem(u32(inc), u32(q), u32(step))
        arr = (PskRx * max(self.nrx, 1))()
        for j, (modem, flags) in enumerate(sel):
            arr[j] = PskRx(_clip(modem), int(flags) & 0xFFFFFFFF)
        h = C.c_void_p()
        check(ddc_lib().pddc_psk_create(C.byref(h), device, self.nrx, _clip(W), self.nmodems,
                                        taps.ctypes.data_as(C.POINTER(C.c_float)), modems, arr))
        self._h = h

    def max_syms(self, n: int) -> int:
        """pddc_psk_max_syms: the most strobes one receiver can have in a batch of n samples (host arithmetic)"""
        c = C.c_size_t()
        check(ddc_lib().pddc_psk_max_syms(self._h, int(n), C.byref(c)))
        return int(c.value)

    def process(self, z, chars=None, counts=None, sym=None, nsym=None, want_sym: bool = False, stream=None):
        """One batch: a complex64 CUDA tensor [nrx, n] whose rows are contiguous (any row stride).  -> (chars, counts) or,
        with want_sym or sym given, (chars, counts, sym, nsym): chars int32 [nrx, capacity, 4], four words per
        pddc_psk_char (`.cpu().numpy().view(psk_char_dtype())[..., 0]` gives the records), of which the first counts[j]
        (int32 [nrx]) of row j are written; sym float32 [nrx, capacity, 2], (d, x) per strobe, of which the first nsym[j]
        (int32 [nrx]) are written.  The outputs, if given, are tensors of these kinds (chars and sym with any capacity
        that suffices); no output may overlap z."""
        n, chars, counts, ccap = self._batch(z, chars, counts)
        scap = 0
        if sym is not None or want_sym:
            import torch
            dev = torch.device("cuda", self.device)
            if sym is None:
                sym = torch.empty((self.nrx, max(self.max_syms(n), 1), 2), dtype=torch.float32, device=dev)
            elif not (sym.dtype == torch.float32 and sym.dim() == 3 and sym.shape[0] == self.nrx and sym.shape[2] == 2
                      and sym[0].is_contiguous()):
                raise PddcError(-1, "psk: sym must be a float32 tensor [nrx, capacity, 2] with contiguous rows")
            if nsym is None:
                nsym = torch.empty((self.nrx,), dtype=torch.int32, device=dev)
            elif not (nsym.dtype == torch.int32 and nsym.dim() == 1 and nsym.shape[0] == self.nrx and nsym.is_contiguous()):
                raise PddcError(-1, "psk: nsym must be a contiguous int32 tensor [nrx]")
            # as for chars: a capacity below the bound must reach the ABI as one (PDDC_ECAPACITY)
            scap = int(sym.stride(0)) // 2 if sym.shape[1] >= self.max_syms(n) else int(sym.shape[1])
        check(ddc_lib().pddc_psk_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)),
                                         chars.data_ptr() if chars.numel() else None, ccap, counts.data_ptr(),
                                         sym.data_ptr() if sym is not None and sym.numel() else None, scap,
                                         nsym.data_ptr() if sym is not None else None, self._stream(stream)))
        return (chars, counts) if sym is None else (chars, counts, sym, nsym)

    def set_rx(self, rx: int, modem: int, flags: int):
        """receiver rx from the next batch's first sample on: PDDC_PSK_RESTART, OFF -> ON or another modem starts it
        afresh (the counters stay)"""
        check(ddc_lib().pddc_psk_set_rx(self._h, int(rx), _clip(modem), int(flags) & 0xFFFFFFFF))

    def read(self, stream=None):
        """-> numpy structured array [nrx] (chars, symbols, acc, reg, d_last, x_last) after the batches submitted so far
        (it waits for them)"""
        return self._read(psk_status_dtype(), stream)


PDDC_SITOR_ON, PDDC_SITOR_REVERSE, PDDC_SITOR_RESTART = 0x1, 0x2, 0x4
PDDC_SITOR_VALID = 0x1
SITOR_ALPHA, SITOR_BETA, SITOR_REPEAT = 0x0F, 0x33, 0x66


def sitor_tile_outputs() -> int:
    """pddc_sitor_tile_outputs: samples per tile of the kernel's walk (tiles begin at the batch's first sample); host
    arithmetic, no device"""
    return int(ddc_lib().pddc_sitor_tile_outputs())


def sitor_char_dtype():
    """pddc_sitor_char as a numpy structured dtype (16 bytes)"""
    import numpy as np
    return np.dtype([("start", np.uint64), ("code", np.uint16), ("flags", np.uint16), ("quality", np.float32)])


def sitor_status_dtype():
    """pddc_sitor_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("chars", np.uint32), ("symbols", np.uint32), ("errors", np.uint32), ("reframes", np.uint32),
                     ("locked", np.uint32), ("acc", np.uint32), ("reg", np.uint32), ("d_last", np.float32)])


def sitor_modem(W: int, samples_per_bit: float, shift: float = 1.7, step: int = None, lock: int = 3, unlock: int = 4):
    """A modem for Sitor's bank at samples_per_bit = rate / baud (8 or more; 100 baud for SITOR-B and NAVTEX).  `shift` is
    the distance of the two tones in units of the baud rate (170 Hz at 100 baud: 1.7); mark lies shift / 2 above the
    receiver's tuned frequency and space as far below it (PDDC_SITOR_REVERSE exchanges them).  The matched filters are
    fsk_modem's: h[t] = w[t] exp(+2 pi i f t), f = +-shift / (2 samples_per_bit) cycles per sample, w a boxcar over
    min(W, round(samples_per_bit)) samples with sum 1 and zero beyond, computed in double and rounded once.  inc =
    round(2^32 / samples_per_bit), at most 2^29; step defaults to inc / 8, an eighth of a sample per transition.
    -> (hm complex64[W], hs complex64[W], inc, step, lock, unlock)"""
    import numpy as np
    W, sps = int(W), float(samples_per_bit)
    if W <= 0 or not sps >= 8.0 or not sps <= float(1 << 32):
        raise PddcError(-1, "sitor_modem: W must be positive and a bit 8 .. 2^32 samples")
    L = min(W, max(1, int(round(sps))))
    t = np.arange(W, dtype=np.float64)
    w = np.where(t < L, 1.0 / L, 0.0)
    f = float(shift) / (2.0 * sps)
    hm, hs = ((w * np.exp(2j * np.pi * g * t)).astype(np.complex64) for g in (f, -f))
    inc = min(max(int(round(float(1 << 32) / sps)), 1), 1 << 29)
    return hm, hs, inc, inc // 8 if step is None else int(step), int(lock), int(unlock)


# The 7-bit constant-ratio code of ITU-R M.476 as this project holds it, the first-received bit lowest, mark (B) = 1;
# unverified against the Recommendation's own text, which was not at hand when this was written.  35 codes, every one of
# weight four: all there are.
_SITOR_LETTERS = {"J": 0x17, "F": 0x1B, "C": 0x1D, "K": 0x1E, "W": 0x27, "Y": 0x2B, "P": 0x2D, "Q": 0x2E, "G": 0x35, "M": 0x39,
                  "X": 0x3A, "V": 0x3C, "A": 0x47, "S": 0x4B, "I": 0x4D, "U": 0x4E, "D": 0x53, "R": 0x55, "E": 0x56, "N": 0x59,
                  " ": 0x5C, "Z": 0x63, "L": 0x65, "H": 0x69, "\n": 0x6C, "O": 0x71, "B": 0x72, "T": 0x74, "\r": 0x78}
_SITOR_LTRS, _SITOR_FIGS, _SITOR_BLANK = 0x5A, 0x36, 0x6A
# code -> the 5-bit ITA2 code of the same character: the text goes through fsk_ita2's tables
_SITOR_ITA2 = {code: _ITA2_LTRS.index(ch) for ch, code in _SITOR_LETTERS.items()}
_SITOR_ITA2.update({_SITOR_LTRS: 31, _SITOR_FIGS: 27, _SITOR_BLANK: 0})
_SITOR_FROM_ITA2 = {v: k for k, v in _SITOR_ITA2.items()}


def sitor_encode(text: str, phasing: int = 16):
    """The mode-B (collective FEC) slot sequence that sends `text`: slots alternate between the DX and the RX position;
    every character goes out in a DX slot and again five slots later in an RX slot, and a slot with nothing to send
    holds phasing signal 2 (beta, DX) or 1 (alpha, RX).  `phasing` pairs of phasing signals come first; three more DX
    slots behind the text carry the last RX copies.  Letters and figures go through the ITA2 tables (the text starts in
    letters; a shift code wherever the table changes).  -> (codes uint8 [slots], bits uint8 [7 slots]: each code's
    first-received bit first, mark = 1).  Host only; what tests and tools key their signals with."""
    import numpy as np
    codes, figs = [], False
    for ch in text.upper():
        here, there = (_ITA2_FIGS, _ITA2_LTRS) if figs else (_ITA2_LTRS, _ITA2_FIGS)
        i = here.find(ch)
        if i <= 0 or i in (27, 31):
            i = there.find(ch)
            if i <= 0 or i in (27, 31):
                raise PddcError(-1, f"sitor_encode: no code for {ch!r}")
            figs = not figs
            codes.append(_SITOR_FIGS if figs else _SITOR_LTRS)
        codes.append(_SITOR_FROM_ITA2[i])
    P, N = max(int(phasing), 0), len(codes)
    slots = np.empty(2 * (P + N) + 6, np.uint8)
    slots[0::2], slots[1::2] = SITOR_BETA, SITOR_ALPHA
    for i, c in enumerate(codes):
        slots[2 * (P + i)] = slots[2 * (P + i) + 5] = c
    bits = ((slots[:, None] >> np.arange(7, dtype=np.uint8)[None, :]) & 1).astype(np.uint8).reshape(-1)
    return slots, bits


def sitor_text(records) -> str:
    """The text of pddc_sitor_char records of one receiver (a numpy array of sitor_char_dtype, or any sequence of records
    with start, code and flags), host only: the receiving side of mode B's time diversity.  The records are put on a
    grid of slots by their start samples (the slot's length is the median distance of two records), so that dropped
    characters do not shift what follows; records off the grid of the last one by more than half a bit -- what a lock
    at a wrong bit phase gave before a phasing word put it right -- are left out; the slot parity that holds beta and, five slots on, what it held before is
    DX; every DX character is paired with the RX one five slots on and whichever of the two is PDDC_SITOR_VALID is
    taken, U+FFFD where neither is; the code is read through the M.476 table and the letters and figures shifts of
    fsk_ita2's tables.  Phasing, repeat and blank signals give no character."""
    import numpy as np
    starts = np.array([int(r["start"]) for r in records], np.int64)
    if starts.size == 0:
        return ""
    codes = [int(r["code"]) for r in records]
    valid = [bool(int(r["flags"]) & PDDC_SITOR_VALID) for r in records]
    gaps = np.diff(starts)
    T = float(np.median(gaps[gaps > 0])) if (gaps > 0).any() else 1.0
    # from the last record back: a record is on the grid if it lies a whole number of slots, to half a bit, in front of
    # the nearest one that is
    at, slot, ahead = {0: starts.size - 1}, 0, int(starts[-1])
    for i in range(starts.size - 2, -1, -1):
        gap = ahead - int(starts[i])
        k = int(round(gap / T))
        if k >= 1 and abs(gap - k * T) <= T / 14.0:
            slot, ahead = slot - k, int(starts[i])
            at[slot] = i
    votes = [0, 0]                                                     # for DX on the even / the odd slots
    for k, i in at.items():
        if not valid[i]:
            continue
        if codes[i] == SITOR_BETA:
            votes[k & 1] += 4
        elif codes[i] == SITOR_ALPHA:
            votes[~k & 1] += 4
        else:
            j = at.get(k + 5)
            if j is not None and valid[j] and codes[j] == codes[i]:
                votes[k & 1] += 1
    dx = 0 if votes[0] >= votes[1] else 1
    out, table = [], _ITA2_LTRS
    first = min(at) - 5
    first += (first ^ dx) & 1
    for k in range(first, max(at) + 1, 2):
        a, b = at.get(k), at.get(k + 5)
        if a is None and b is None:
            continue
        if a is not None and valid[a]:
            c = codes[a]
        elif b is not None and valid[b]:
            c = codes[b]
        else:
            out.append("�")
            continue
        c = _SITOR_ITA2.get(c)
        if c is None or c == 0:                                        # alpha, beta, repeat; blank
            continue
        if c == 27:
            table = _ITA2_FIGS
        elif c == 31:
            table = _ITA2_LTRS
        else:
            out.append(table[c])
    return "".join(out)


class Sitor(_Decoder):
    """pddc_sitor: synchronous FSK (SITOR-B, NAVTEX, AMTOR FEC) decoding of every receiver's complex series, such as Tuner,
    Blanker, RxFilter or Carrier write, on the device (include/perseus_ddc.h): fsk's two matched filters of W complex
    taps, a bit clock that every transition corrects, and the framing of the 7-bit constant-ratio code by the phasing
    signals per receiver; the output is 7-bit characters, which sitor_text turns into text on the host.
    bank: up to 16 modems (hm, hs, inc, step, lock, unlock), as sitor_modem gives them, every hm and hs of W taps; sel:
    one (modem, flags) per receiver, flags PDDC_SITOR_ON | PDDC_SITOR_REVERSE.  Feed it every batch in order on one
    stream; every output bit is the same however the series is cut."""
    _kind = "sitor"

    def __init__(self, bank, sel, W: int, device: int = 0):
        import numpy as np
        bank = [tuple(b) for b in bank]
        sel = [tuple(r) for r in sel]
        self.W, self.nrx, self.nmodems, self.device = int(W), len(sel), len(bank), device
        taps = np.zeros((max(self.nmodems, 1), 2, max(self.W, 1)), np.complex64)
        modems = (SitorModem * max(self.nmodems, 1))()
        u32 = lambda v: max(0, min(int(v), (1 << 32) - 1))
        for b, (hm, hs, inc, step, lock, unlock) in enumerate(bank):
            for i, h in enumerate((hm, hs)):
                h = np.asarray(h, dtype=np.complex64).reshape(-1)
                if h.size != self.W:
                    raise PddcError(-1, f"sitor: modem {b}: {h.size} taps for a window of {self.W}")
                taps[b, i] = h
            modems[b] = SitorModem(u32(inc), u32(step), u32(lock), u32(unlock))
        arr = (SitorRx * max(self.nrx, 1))()
        for j, (modem, flags) in enumerate(sel):
            arr[j] = SitorRx(_clip(modem), int(flags) & 0xFFFFFFFF)
        h = C.c_void_p()
        check(ddc_lib().pddc_sitor_create(C.byref(h), device, self.nrx, _clip(W), self.nmodems,
                                          taps.ctypes.data_as(C.POINTER(C.c_float)), modems, arr))
        self._h = h

    def max_syms(self, n: int) -> int:
        """pddc_sitor_max_syms: the most strobes one receiver can have in a batch of n samples (host arithmetic)"""
        c = C.c_size_t()
        check(ddc_lib().pddc_sitor_max_syms(self._h, int(n), C.byref(c)))
        return int(c.value)

    def process(self, z, chars=None, counts=None, soft=None, nsoft=None, want_soft: bool = False, stream=None):
        """One batch: a complex64 CUDA tensor [nrx, n] whose rows are contiguous (any row stride).  -> (chars, counts) or,
        with want_soft or soft given, (chars, counts, soft, nsoft): chars int32 [nrx, capacity, 4], four words per
        pddc_sitor_char (`.cpu().numpy().view(sitor_char_dtype())[..., 0]` gives the records), of which the first
        counts[j] (int32 [nrx]) of row j are written; soft float32 [nrx, capacity], d at every strobe, of which the first
        nsoft[j] (int32 [nrx]) are written.  The outputs, if given, are tensors of these kinds (chars and soft with any
        capacity that suffices); no output may overlap z."""
        n, chars, counts, ccap = self._batch(z, chars, counts)
        scap = 0
        if soft is not None or want_soft:
            import torch
            soft, scap = self._out(soft, max(self.max_syms(n), 1) if soft is None else self.max_syms(n), torch.float32,
                                   "soft must be a float32")
            if nsoft is None:
                nsoft = torch.empty((self.nrx,), dtype=torch.int32, device=torch.device("cuda", self.device))
            elif not (nsoft.dtype == torch.int32 and nsoft.dim() == 1 and nsoft.shape[0] == self.nrx and nsoft.is_contiguous()):
                raise PddcError(-1, "sitor: nsoft must be a contiguous int32 tensor [nrx]")
        check(ddc_lib().pddc_sitor_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)),
                                           chars.data_ptr() if chars.numel() else None, ccap, counts.data_ptr(),
                                           soft.data_ptr() if soft is not None and soft.numel() else None, scap,
                                           nsoft.data_ptr() if soft is not None else None, self._stream(stream)))
        return (chars, counts) if soft is None else (chars, counts, soft, nsoft)

    def set_rx(self, rx: int, modem: int, flags: int):
        """receiver rx from the next batch's first sample on: PDDC_SITOR_RESTART, or OFF -> ON, starts it afresh (the
        counters stay); another modem keeps the carried inputs and the clock and starts the framing afresh"""
        check(ddc_lib().pddc_sitor_set_rx(self._h, int(rx), _clip(modem), int(flags) & 0xFFFFFFFF))

    def read(self, stream=None):
        """-> numpy structured array [nrx] (chars, symbols, errors, reframes, locked, acc, reg, d_last) after the batches
        submitted so far (it waits for them)"""
        return self._read(sitor_status_dtype(), stream)


PDDC_FAX_ON, PDDC_FAX_REVERSE, PDDC_FAX_RESTART = 0x1, 0x2, 0x4
PDDC_FAX_START, PDDC_FAX_STOP, PDDC_FAX_ACTIVE = 0x1, 0x2, 0x4


def fax_tile_outputs() -> int:
    """pddc_fax_tile_outputs: samples per tile of the kernel's walk (tiles begin at the batch's first sample); host
    arithmetic, no device"""
    return int(ddc_lib().pddc_fax_tile_outputs())


def fax_line_dtype():
    """pddc_fax_line as a numpy structured dtype (16 bytes)"""
    import numpy as np
    return np.dtype([("start", np.uint64), ("crossings", np.uint16), ("white", np.uint16), ("flags", np.uint16), ("run", np.uint16)])


def fax_status_dtype():
    """pddc_fax_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("lines", np.uint32), ("pixels", np.uint32), ("images", np.uint32), ("active", np.uint32), ("acc", np.uint32),
                     ("col", np.uint32), ("f_last", np.float32)])


def _fax_tone_range(hz: float, lpm: float, tol: float):
    """the crossings a line of a tone of `hz` has, `tol` either way, as whole numbers that contain them"""
    import math
    c = float(hz) * 60.0 / float(lpm)
    return max(int(math.floor(c * (1.0 - tol))), 0), min(int(math.ceil(c * (1.0 + tol))), 65535)


def fax_modem(rate_hz: float, W: int, lpm: float = 120.0, ioc: int = 576, deviation_hz: float = 400.0, width: int = None,
              start_hz: float = None, stop_hz: float = 450.0, need: int = 4, tone_tol: float = 0.1, box: int = None, beta: float = 5.0,
              cutoff_hz: float = None):
    """A modem for Fax's bank at a receiver rate of rate_hz, the receiver tuned to the subcarrier's centre (1900 Hz of the
    audio): black lies deviation_hz below it and white as far above.  width = round(pi ioc) pixels per line unless given;
    inc = round(2^32 width lpm / 60 / rate_hz), at most 2^31; box = the samples per pixel, rounded, 1 .. 16.  The taps are
    a Kaiser-windowed (beta) low-pass of W taps whose -6 dB edge lies at cutoff_hz (at most 0.45 rate_hz), sum 1, computed
    in double and rounded once.  cutoff_hz defaults to deviation_hz plus an eighth of the pixel rate: the deviation plus
    half the pixel rate, which passes detail down to single pixels, leaves so much of the discriminator's noise (it grows
    with the square of the frequency) that at a carrier 20 dB above the noise a flat grey is off by 55 levels; at an
    eighth it is off by less than 32 (tests/test_fax_cpu.py) and detail of 8 pixels and more keeps its contrast.  scale and bias put f = -+2 deviation_hz / rate_hz on 0 and
    255.  The start tone is 300 Hz for IOC 576 and 675 Hz for IOC 288 unless given, the stop tone 450 Hz: a line of a
    tone has tone 60 / lpm crossings, and the ranges take tone_tol either way; `need` such lines in a row start or stop
    an image.  -> (h float32[W], inc, width, box, scale, bias, start_lo, start_hi, stop_lo, stop_hi, need)"""
    import numpy as np
    W, rate, lpm = int(W), float(rate_hz), float(lpm)
    if W <= 0 or not rate > 0.0 or not lpm > 0.0 or not float(deviation_hz) > 0.0:
        raise PddcError(-1, "fax_modem: W, the rate, the lines per minute and the deviation must be positive")
    width = int(round(np.pi * int(ioc))) if width is None else int(width)
    pixel_rate = width * lpm / 60.0
    spp = rate / pixel_rate
    if not spp >= 2.0:
        raise PddcError(-1, f"fax_modem: {spp:.3f} samples per pixel, a pixel needs 2")
    inc = min(max(int(round(4294967296.0 / spp)), 1), 1 << 31)
    box = min(max(int(round(spp)), 1), 16) if box is None else int(box)
    cutoff_hz = float(deviation_hz) + 0.125 * pixel_rate if cutoff_hz is None else float(cutoff_hz)
    fc = min(cutoff_hz, 0.45 * rate) / rate                                       # cycles per sample
    t = np.arange(W, dtype=np.float64) - 0.5 * (W - 1)
    h = 2.0 * fc * np.sinc(2.0 * fc * t) * np.kaiser(W, float(beta))
    h = (h / h.sum()).astype(np.float32)
    fd = 2.0 * float(deviation_hz) / rate
    if start_hz is None:
        start_hz = 675.0 if int(ioc) == 288 else 300.0
    s_lo, s_hi = _fax_tone_range(start_hz, lpm, tone_tol)
    p_lo, p_hi = _fax_tone_range(stop_hz, lpm, tone_tol)
    return h, inc, width, box, float(np.float32(127.5 / fd)), 127.5, s_lo, s_hi, p_lo, p_hi, int(need)


def fax_encode(image, modem, rate_hz: float, start_lines: int = 10, phasing_lines: int = 20, stop_lines: int = 10, lead: int = 0,
               deviation_hz: float = 400.0, trail_lines: int = 1):
    """The complex series of a whole transmission of `image` (uint8 [rows, width], 0 black, 255 white) as a receiver tuned
    to the subcarrier's centre sees it: `lead` black pixels (the receiver's line grid is not the sender's), start_lines of
    the start tone, phasing_lines (white for the first twentieth of the line, black behind it), the image, stop_lines of
    the stop tone and trail_lines of black.  The tones are square waves of black and white with as many periods per line
    as lie in the middle of the modem's ranges.  A sample's pixel is the one the modem's own clock is in, floor(m inc /
    2^32); its frequency lies (pixel / 255 - 1 / 2) 2 deviation_hz from the centre, and the phase is continuous.  Host
    only; what tests and tools make their signals with.  -> complex64 [samples]"""
    import numpy as np
    h, inc, width, box, scale, bias, s_lo, s_hi, p_lo, p_hi, need = modem
    img = np.asarray(image, dtype=np.uint8)
    if img.ndim != 2 or img.shape[1] != int(width):
        raise PddcError(-1, f"fax_encode: the image must be [rows, {int(width)}]")
    col = np.arange(int(width), dtype=np.float64)

    def tone(lo, hi):
        cycles = 0.5 * (int(lo) + int(hi))
        return np.where((col * cycles / int(width)) % 1.0 < 0.5, 255, 0).astype(np.uint8)
    phasing = np.where(col < max(int(width) // 20, 1), 255, 0).astype(np.uint8)
    rows = ([tone(s_lo, s_hi)] * int(start_lines) + [phasing] * int(phasing_lines) + list(img) + [tone(p_lo, p_hi)] * int(stop_lines)
            + [np.zeros(int(width), np.uint8)] * int(trail_lines))
    pixels = np.concatenate([np.zeros(int(lead), np.uint8)] + rows)
    n = int((pixels.size << 32) // int(inc))                           # the samples whose pixel exists
    at = (np.arange(n, dtype=np.uint64) * np.uint64(int(inc))) >> np.uint64(32)
    freq = (pixels[at].astype(np.float64) / 255.0 - 0.5) * 2.0 * float(deviation_hz) / float(rate_hz)
    phase = 2.0 * np.pi * np.cumsum(freq)
    return np.exp(1j * phase).astype(np.complex64)


def fax_image(records, pixels, width: int):
    """The pictures in one receiver's output, host only: `records` its pddc_fax_line records of all batches (a numpy
    array of fax_line_dtype) and `pixels` its pixels of all batches, from a point where the receiver was fresh or
    restarted, so that record k closes pixels k width .. (k + 1) width - 1.  A picture begins behind the line where a
    START run reached `need` (run == need; the start-tone lines that follow are skipped) and ends in front of the STOP
    run whose run reached `need`.  The lines in front that hold a short white pulse (white in at most an eighth of the
    line, at most two crossings; up to two lines that the start tone ends in are passed over) are the phasing lines: the column where their pulse begins, the median over them, is
    where the sender's lines begin, and every line of the picture is rotated by it; a line then runs over two of the
    receiver's lines, and the picture has one line less than the records between.  -> a list of (picture uint8 [rows,
    width], column, phasing lines found), one per image; a transmission without its stop tone gives none."""
    import numpy as np
    width = int(width)
    rec = np.asarray(records)
    px = np.asarray(pixels, dtype=np.uint8).reshape(-1)
    nl = min(int(rec.shape[0]), px.size // width)
    flags, run = rec["flags"][:nl].astype(np.int64), rec["run"][:nl].astype(np.int64)
    out, k = [], 0

    def pulse(i):
        line = px[i * width:(i + 1) * width] >= 128
        return line if 0 < int(line.sum()) <= width // 8 and int(rec["crossings"][i]) <= 2 else None
    while k < nl:
        # the line where a START run begins to count as one: ACTIVE rises there
        if not (flags[k] & PDDC_FAX_START and flags[k] & PDDC_FAX_ACTIVE and (k == 0 or not flags[k - 1] & PDDC_FAX_ACTIVE)):
            k += 1
            continue
        first = k + 1
        while first < nl and flags[first] & PDDC_FAX_START:
            first += 1
        end = first
        while end < nl and flags[end] & PDDC_FAX_ACTIVE:
            end += 1
        if end >= nl:
            break
        last = end - int(run[end]) + 1                                  # the first line of the STOP run that ended it
        ph = first
        while ph < min(first + 2, last) and pulse(ph) is None:         # the line the start tone ends in
            ph += 1
        cols = []
        while ph < last and pulse(ph) is not None:
            line = pulse(ph)
            cols.append(int(np.flatnonzero(line & ~np.roll(line, 1))[0]))
            ph += 1
        if not cols:
            ph = first
        col = int(np.median(cols)) if cols else 0
        body = px[ph * width + col:(last - 1) * width + col] if col else px[ph * width:last * width]
        out.append((body.reshape(-1, width).copy(), col, len(cols)))
        k = end
    return out


class Fax(_Decoder):
    """pddc_fax: radiofax (WEFAX) decoding of every receiver's complex series, such as Tuner, Blanker, RxFilter or Carrier
    write, on the device (include/perseus_ddc.h): a real low-pass of W taps, an FM discriminator, a free-running pixel
    clock, a boxcar and a grey map per receiver; the output is pixels and one record per line (its start sample, its
    crossings and white count, start / stop tone and whether an image is in progress), which fax_image turns into
    pictures on the host.  bank: up to 16 modems as fax_modem gives them, every h of W taps; sel: one (modem, flags) per
    receiver, flags PDDC_FAX_ON | PDDC_FAX_REVERSE.  Feed it every batch in order on one stream; every output bit is
    the same however the series is cut."""
    _kind = "fax"
    _bound = "max_lines"

    def __init__(self, bank, sel, W: int, device: int = 0):
        import numpy as np
        bank = [tuple(b) for b in bank]
        sel = [tuple(r) for r in sel]
        self.W, self.nrx, self.nmodems, self.device = int(W), len(sel), len(bank), device
        taps = np.zeros((max(self.nmodems, 1), max(self.W, 1)), np.float32)
        modems = (FaxModem * max(self.nmodems, 1))()
        u32 = lambda v: max(0, min(int(v), (1 << 32) - 1))
        u16 = lambda v: max(0, min(int(v), 65535))
        for b, (h, inc, width, box, scale, bias, s_lo, s_hi, p_lo, p_hi, need) in enumerate(bank):
            h = np.asarray(h, dtype=np.float32).reshape(-1)
            if h.size != self.W:
                raise PddcError(-1, f"fax: modem {b}: {h.size} taps for a window of {self.W}")
            taps[b] = h
            modems[b] = FaxModem(u32(inc), u32(width), u32(box), float(scale), float(bias), u16(s_lo), u16(s_hi), u16(p_lo), u16(p_hi),
                                 u32(need))
        arr = (FaxRx * max(self.nrx, 1))()
        for j, (modem, flags) in enumerate(sel):
            arr[j] = FaxRx(_clip(modem), int(flags) & 0xFFFFFFFF)
        h = C.c_void_p()
        check(ddc_lib().pddc_fax_create(C.byref(h), device, self.nrx, _clip(W), self.nmodems,
                                        taps.ctypes.data_as(C.POINTER(C.c_float)), modems, arr))
        self._h = h

    max_lines = _Decoder.max_chars

    def max_pixels(self, n: int) -> int:
        """pddc_fax_max_pixels: the most strobes one receiver can have in a batch of n samples (host arithmetic)"""
        c = C.c_size_t()
        check(ddc_lib().pddc_fax_max_pixels(self._h, int(n), C.byref(c)))
        return int(c.value)

    def process(self, z, pix=None, npix=None, lines=None, counts=None, disc=None, want_disc: bool = False, stream=None):
        """One batch: a complex64 CUDA tensor [nrx, n] whose rows are contiguous (any row stride).  -> (pix, npix, lines,
        counts) or, with want_disc or disc given, (pix, npix, lines, counts, disc): pix uint8 [nrx, capacity] of which the
        first npix[j] (int32 [nrx]) of row j are written; lines int32 [nrx, capacity, 4], four words per pddc_fax_line
        (`.cpu().numpy().view(fax_line_dtype())[..., 0]` gives the records), of which the first counts[j] (int32 [nrx])
        are written; disc float32 [nrx, n or more], f of every sample.  The outputs, if given, are tensors of these kinds
        (pix and lines with any capacity that suffices); no output may overlap z."""
        import torch
        n, lines, counts, lcap = self._batch(z, lines, counts)
        bound = self.max_pixels(n)
        pix, pcap = self._out(pix, max(bound, 1) if pix is None else bound, torch.uint8, "pix must be a uint8")
        if npix is None:
            npix = torch.empty((self.nrx,), dtype=torch.int32, device=torch.device("cuda", self.device))
        elif not (npix.dtype == torch.int32 and npix.dim() == 1 and npix.shape[0] == self.nrx and npix.is_contiguous()):
            raise PddcError(-1, "fax: npix must be a contiguous int32 tensor [nrx]")
        dcap = 0
        if disc is not None or want_disc:
            disc, dcap = self._out(disc, max(n, 1) if disc is None else n, torch.float32, "disc must be a float32")
        check(ddc_lib().pddc_fax_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)),
                                         pix.data_ptr() if pix.numel() else None, pcap, npix.data_ptr(),
                                         lines.data_ptr() if lines.numel() else None, lcap, counts.data_ptr(),
                                         disc.data_ptr() if disc is not None and disc.numel() else None, dcap, self._stream(stream)))
        return (pix, npix, lines, counts) if disc is None else (pix, npix, lines, counts, disc)

    def set_rx(self, rx: int, modem: int, flags: int):
        """receiver rx from the next batch's first sample on: PDDC_FAX_RESTART, or OFF -> ON, starts it afresh (the
        counters stay); another modem keeps the carried inputs, the discriminator and the clock and starts the line afresh"""
        check(ddc_lib().pddc_fax_set_rx(self._h, int(rx), _clip(modem), int(flags) & 0xFFFFFFFF))

    def read(self, stream=None):
        """-> numpy structured array [nrx] (lines, pixels, images, active, acc, col, f_last) after the batches submitted so
        far (it waits for them)"""
        return self._read(fax_status_dtype(), stream)


PDDC_MFSK_ON, PDDC_MFSK_REVERSE, PDDC_MFSK_RESTART = 0x1, 0x2, 0x4
PDDC_MFSK_MAX_TONES = 32


def mfsk_tile_outputs() -> int:
    """pddc_mfsk_tile_outputs: samples per tile of the kernel's walk (tiles begin at the batch's first sample); host
    arithmetic, no device"""
    return int(ddc_lib().pddc_mfsk_tile_outputs())


def mfsk_sym_dtype():
    """pddc_mfsk_sym as a numpy structured dtype (16 bytes)"""
    import numpy as np
    return np.dtype([("start", np.uint64), ("tone", np.uint8), ("second", np.uint8), ("flags", np.uint16), ("quality", np.float32)])


def mfsk_status_dtype():
    """pddc_mfsk_status as a numpy structured dtype"""
    import numpy as np
    return np.dtype([("symbols", np.uint32), ("acc", np.uint32), ("skip", np.uint32), ("tone_last", np.uint32), ("q_last", np.float32)])


def mfsk_modem(rate_hz: float, baud: float, tone0_hz: float, spacing_hz: float, ntones: int, W: int, q: int = None, step: int = None,
               window: str = "rect"):
    """A modem for Mfsk's bank: tone k = 0 .. ntones - 1 lies at f_k = tone0_hz + k spacing_hz (offsets from the receiver's
    tuned frequency, either sign) and its matched filter is h_k[t] = w[t] exp(+2 pi i f_k t / rate_hz) over one symbol, L =
    min(W, round(rate_hz / baud)) samples: w a boxcar ("rect": tones a baud apart are orthogonal) or a Hann window
    ("hann": tones two bauds apart are, and far ones leak less), of unit sum and zero beyond L, computed in double and
    rounded once.  The filter's output peaks where the window covers the symbol: L - 1 samples behind its first sample.
    inc = round(2^32 baud / rate_hz), at most 2^29; q = round(a quarter symbol) in 1 .. 64 with 4 q inc <= 2^32; step
    defaults to inc // 64, a 64th of a sample per strobe (inc is one sample of the clock): what it follows is a clock
    error of 1 / (64 samples per symbol), so long symbols want a larger step.
    -> (h complex64 [ntones, W], inc, q, step, tone0_hz, spacing_hz): Mfsk takes the first four, mfsk_encode all six"""
    import numpy as np
    W, M, rate, baud = int(W), int(ntones), float(rate_hz), float(baud)
    if W <= 0 or not 2 <= M <= PDDC_MFSK_MAX_TONES or not rate > 0.0 or not baud > 0.0 or not rate >= 8.0 * baud:
        raise PddcError(-1, "mfsk_modem: W positive, 2 .. 32 tones, and a symbol of 8 samples or more")
    if window not in ("rect", "hann"):
        raise PddcError(-1, "mfsk_modem: window is \"rect\" or \"hann\"")
    sps = rate / baud
    L = min(W, max(1, int(round(sps))))
    t = np.arange(W, dtype=np.float64)
    w = np.where(t < L, 1.0 if window == "rect" else 1.0 - np.cos(2.0 * np.pi * (t + 0.5) / L), 0.0)
    w = w / w.sum()
    f = float(tone0_hz) + float(spacing_hz) * np.arange(M, dtype=np.float64)
    h = (w[None, :] * np.exp(2j * np.pi * (f / rate)[:, None] * t[None, :])).astype(np.complex64)
    inc = min(max(int(round(4294967296.0 / sps)), 1), 1 << 29)
    q = int(round(sps / 4.0)) if q is None else int(q)
    q = min(max(q, 1), 64)
    while q > 1 and 4 * q * inc > (1 << 32):
        q -= 1
    return h, inc, q, inc // 64 if step is None else int(step), float(tone0_hz), float(spacing_hz)


def mfsk_encode(tones, modem, rate_hz: float, lead: float = 0.0, ppm: float = 0.0, n: int = None, amplitude: float = 1.0):
    """The series a sender of `tones` (a sequence of tone numbers) gives a receiver on `modem` (mfsk_modem's six), for tests
    and tools, host only: symbol k lasts T = 2^32 / inc (1 + ppm 1e-6) samples from sample lead + k T on and has the
    frequency tone0_hz + tones[k] spacing_hz; the phase runs on from symbol to symbol (continuous-phase FSK), the
    amplitude is constant over the symbols and zero outside them.  n: the length, default the symbols and one more.
    -> complex64 [n]"""
    import numpy as np
    h, inc, _, _, tone0, spacing = modem
    tones = np.asarray(tones, dtype=np.int64).reshape(-1)
    if tones.size and (tones.min() < 0 or tones.max() >= np.asarray(h).shape[0]):
        raise PddcError(-1, "mfsk_encode: a tone the modem does not have")
    T = 4294967296.0 / float(inc) * (1.0 + float(ppm) * 1e-6)
    if n is None:
        n = int(np.ceil(float(lead) + (tones.size + 1) * T))
    k = np.floor((np.arange(n, dtype=np.float64) - float(lead)) / T).astype(np.int64)
    inside = (k >= 0) & (k < tones.size)
    f = np.where(inside, tone0 + spacing * tones[np.clip(k, 0, max(tones.size - 1, 0))] if tones.size else 0.0, 0.0)
    phase = np.concatenate([[0.0], np.cumsum(f[:-1])]) / float(rate_hz) if n else np.zeros(0)
    return (float(amplitude) * inside * np.exp(2j * np.pi * (phase - np.floor(phase)))).astype(np.complex64)


class Mfsk(_Decoder):
    """pddc_mfsk: M-tone FSK (2G ALE, MFSK16 / 8, the tone layer of Olivia and Contestia) symbol decoding of every
    receiver's complex series, such as Tuner, Blanker, RxFilter or Carrier write, on the device (include/perseus_ddc.h):
    M complex matched filters of W taps, the strongest and the second strongest tone of every sample, and a symbol clock
    that looks a quarter symbol to either side of the decision; the output is one record per symbol (start, tone,
    second, quality), which ale_words and its like read on the host.
    bank: up to 16 modems (h [M, W], inc, q, step, ...), as mfsk_modem gives them; sel: one (modem, flags) per receiver,
    flags PDDC_MFSK_ON | PDDC_MFSK_REVERSE.  Feed it every batch in order on one stream; every output bit is the same
    however the series is cut."""
    _kind = "mfsk"
    _bound = "max_syms"

    def __init__(self, bank, sel, W: int, device: int = 0):
        import numpy as np
        bank = [tuple(b)[:4] for b in bank]
        sel = [tuple(r) for r in sel]
        self.W, self.nrx, self.nmodems, self.device = int(W), len(sel), len(bank), device
        taps = np.zeros((max(self.nmodems, 1), PDDC_MFSK_MAX_TONES, max(self.W, 1)), np.complex64)
        modems = (MfskModem * max(self.nmodems, 1))()
        u32 = lambda v: max(0, min(int(v), (1 << 32) - 1))
        for b, (h, inc, q, step) in enumerate(bank):
            h = np.asarray(h, dtype=np.complex64)
            if h.ndim != 2 or h.shape[1] != self.W or h.shape[0] > PDDC_MFSK_MAX_TONES:
                raise PddcError(-1, f"mfsk: modem {b}: taps {h.shape} for a window of {self.W} and at most {PDDC_MFSK_MAX_TONES} tones")
            taps[b, :h.shape[0]] = h
            modems[b] = MfskModem(h.shape[0], u32(inc), u32(q), u32(step))
        arr = (MfskRx * max(self.nrx, 1))()
        for j, (modem, flags) in enumerate(sel):
            arr[j] = MfskRx(_clip(modem), int(flags) & 0xFFFFFFFF)
        h = C.c_void_p()
        check(ddc_lib().pddc_mfsk_create(C.byref(h), device, self.nrx, _clip(W), self.nmodems,
                                         taps.ctypes.data_as(C.POINTER(C.c_float)), modems, arr))
        self._h = h

    max_syms = _Decoder.max_chars

    def process(self, z, syms=None, counts=None, best=None, want_best: bool = False, stream=None):
        """One batch: a complex64 CUDA tensor [nrx, n] whose rows are contiguous (any row stride).  -> (syms, counts) or,
        with want_best or best given, (syms, counts, best): syms int32 [nrx, capacity, 4], four words per pddc_mfsk_sym
        (`.cpu().numpy().view(mfsk_sym_dtype())[..., 0]` gives the records), of which the first counts[j] (int32 [nrx])
        of row j are written; best float32 [nrx, n], the strongest tone's power at every sample.  syms, counts and best,
        if given, are tensors of these kinds (syms and best with any capacity that suffices); no output may overlap z."""
        n, syms, counts, scap = self._batch(z, syms, counts)
        bcap = 0
        if best is not None or want_best:
            import torch
            best, bcap = self._out(best, n, torch.float32, "best must be a float32")
        check(ddc_lib().pddc_mfsk_process(self._h, z.data_ptr() if n else None, n, int(z.stride(0)),
                                          syms.data_ptr() if syms.numel() else None, scap, counts.data_ptr(),
                                          best.data_ptr() if best is not None and best.numel() else None, bcap, self._stream(stream)))
        return (syms, counts) if best is None else (syms, counts, best[:, :n])

    def set_rx(self, rx: int, modem: int, flags: int):
        """receiver rx from the next batch's first sample on: PDDC_MFSK_RESTART, OFF -> ON or another modem starts it
        afresh (the counter stays)"""
        check(ddc_lib().pddc_mfsk_set_rx(self._h, int(rx), _clip(modem), int(flags) & 0xFFFFFFFF))

    def read(self, stream=None):
        """-> numpy structured array [nrx] (symbols, acc, skip, tone_last, q_last) after the batches submitted so far (it waits
        for them)"""
        return self._read(mfsk_status_dtype(), stream)


# ---- 2G ALE (MIL-STD-188-141A) on the host: words from Mfsk's symbol records -------------------------------------------
# The Golay generator, the bit order within a symbol and a word, the interleaving and the inverted half below are this
# project's own statement from memory, NOT verified against the standard's text: ale_encode and ale_words agree with each
# other (the tests are round trips), and an on-air signal may need one of the conventions turned round.

ALE_PREAMBLES = ("DATA", "THRU", "TO", "TWS", "FROM", "TIS", "CMD", "REP")
ALE_BASIC38 = "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789@?"
ALE_WORD_SYMBOLS = 49
_ALE_GRAY = (0b000, 0b001, 0b011, 0b010, 0b110, 0b111, 0b101, 0b100)
_ALE_GOLAY_POLY = 0xC75                                 # x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1
_ale_golay_table = None


def ale_modem(rate_hz: float, W: int, q: int = None, step: int = None):
    """mfsk_modem for 2G ALE: 8 tones 750 .. 2500 Hz, 250 Hz apart, 125 baud, Hann-windowed filters (the tones are two
    bauds apart).  step defaults to inc // 2, half a sample per strobe: at 78 samples a symbol mfsk_modem's 64th of a
    sample would not follow a sender 200 ppm off"""
    h, inc, q, _, tone0, spacing = mfsk_modem(rate_hz, 125.0, 750.0, 250.0, 8, W, q=q, step=0, window="hann")
    return h, inc, q, inc // 2 if step is None else int(step), tone0, spacing


def ale_tribits(tones):
    """The three bits of each tone, the first highest, by ALE's Gray map: tone 0 .. 7 -> 000, 001, 011, 010, 110, 111,
    101, 100.  -> a list of 0 / 1, three per tone"""
    out = []
    for t in tones:
        g = _ALE_GRAY[int(t) & 7]
        out += [g >> 2 & 1, g >> 1 & 1, g & 1]
    return out


def ale_golay_check(data12: int) -> int:
    """The 12 check bits of the extended Golay (24, 12) code for 12 data bits: the remainder of data x^11 by the
    generator (11 bits), then an even parity bit over the 23"""
    r = (int(data12) & 0xFFF) << 11
    for i in range(22, 10, -1):
        if r >> i & 1:
            r ^= _ALE_GOLAY_POLY << (i - 11)
    r &= 0x7FF
    return r << 1 | (bin((int(data12) & 0xFFF) << 11 | r).count("1") & 1)


def ale_golay_decode(word24: int):
    """A received codeword (12 data bits, then 12 check bits) -> (data12, errors corrected) or None where more than
    3 bits are wrong (the code's distance is 8: every pattern of up to 3 errors is corrected, none of 4 miscorrected)"""
    global _ale_golay_table
    if _ale_golay_table is None:
        from itertools import combinations
        table = {0: 0}
        for w in (1, 2, 3):
            for bits in combinations(range(24), w):
                e = sum(1 << b for b in bits)
                table[ale_golay_check(e >> 12) ^ (e & 0xFFF)] = e
        _ale_golay_table = table
    word24 = int(word24) & 0xFFFFFF
    e = _ale_golay_table.get(ale_golay_check(word24 >> 12) ^ (word24 & 0xFFF))
    return None if e is None else ((word24 ^ e) >> 12, bin(e).count("1"))


def ale_encode(words):
    """The tones of ALE words, 49 per word.  words: (preamble, three characters) pairs, the preamble a name of
    ALE_PREAMBLES or its number, the characters of ALE_BASIC38 -- ("TO", "ABC").  A word is 24 bits, the preamble's
    three and three 7-bit ASCII characters, the first bit highest; its halves A and B become Golay codewords, B's check
    bits inverted; the 48 bits go out interleaved A1 B1 A2 B2 ... with a stuff bit 0 behind, three times over: 147 bits,
    49 tones of three bits.  -> a list of tone numbers"""
    bits = []
    for pre, chars in words:
        p = ALE_PREAMBLES.index(pre) if isinstance(pre, str) else int(pre)
        if not 0 <= p < 8 or len(chars) != 3 or any(c not in ALE_BASIC38 for c in chars):
            raise PddcError(-1, f"ale_encode: ({pre!r}, {chars!r}) is no ALE word")
        w = p << 21 | ord(chars[0]) << 14 | ord(chars[1]) << 7 | ord(chars[2])
        a, b = w >> 12, w & 0xFFF
        ca, cb = a << 12 | ale_golay_check(a), b << 12 | (ale_golay_check(b) ^ 0xFFF)
        one = []
        for i in range(23, -1, -1):
            one += [ca >> i & 1, cb >> i & 1]
        bits += (one + [0]) * 3
    inverse = {g: t for t, g in enumerate(_ALE_GRAY)}
    return [inverse[bits[i] << 2 | bits[i + 1] << 1 | bits[i + 2]] for i in range(0, len(bits), 3)]


def ale_words(records):
    """The ALE words in a receiver's symbols: pddc_mfsk_sym records (a numpy array of mfsk_sym_dtype) or plain tone
    numbers.  It slides over them; at every offset it takes 49 symbols = 147 bits, votes 2 of 3 over bits i, i + 49 and
    i + 98, drops the stuff bit, de-interleaves, restores the inverted check bits of the second codeword and
    Golay-decodes both halves with up to 3 errors each.  A word is accepted when both decode and its three characters
    are of ALE_BASIC38.  -> a list of dicts {start: the first symbol's start (its index for plain tones), preamble,
    chars, errors: the bits the two decoders corrected, split: of the 49 votes those that were not unanimous}.
    That rule alone accepts about one wrong offset in a hundred -- there the three copies are those of two neighbouring
    words, and what they vote into decodes as often as random bits do (2325 of 4096 syndromes, twice, and 38 of 128
    characters, three times): such words have errors of 4 .. 6 and many split votes, and do not lie 49 symbols from the
    next one.  A caller that wants none of them keeps the words with split = 0 or chains them by their starts."""
    import numpy as np
    rec = np.asarray(records)
    named = rec.dtype.names is not None
    tones = (rec["tone"] if named else rec).astype(np.int64).reshape(-1)
    starts = rec["start"].reshape(-1) if named else np.arange(tones.size)
    gray = np.array(_ALE_GRAY, np.int64)[tones & 7]
    bits = np.stack([gray >> 2 & 1, gray >> 1 & 1, gray & 1], axis=1).reshape(-1)
    weights = 1 << np.arange(23, -1, -1, dtype=np.int64)
    out = []
    for o in range(0, tones.size - ALE_WORD_SYMBOLS + 1):
        b = bits[3 * o:3 * o + 147].reshape(3, 49)
        votes = b.sum(axis=0)
        v = (votes >= 2).astype(np.int64)[:48]
        ca, cb = int(v[0::2] @ weights), int(v[1::2] @ weights) ^ 0xFFF
        da, db = ale_golay_decode(ca), ale_golay_decode(cb)
        if da is None or db is None:
            continue
        w = da[0] << 12 | db[0]
        chars = "".join(chr(w >> s & 0x7F) for s in (14, 7, 0))
        if all(c in ALE_BASIC38 for c in chars):
            out.append({"start": int(starts[o]), "preamble": ALE_PREAMBLES[w >> 21], "chars": chars, "errors": da[1] + db[1],
                        "split": int(((votes != 0) & (votes != 3)).sum())})
    return out


def ale_text(words) -> str:
    """The addresses in ale_words' words: a DATA or REP word carries on the address of the word before it, any other
    preamble begins one; the fill character @ is dropped.  -> "TO ABCDEF TIS XYZ" """
    parts = []
    for w in words:
        chars = w["chars"].replace("@", "")
        if w["preamble"] in ("DATA", "REP") and parts:
            parts[-1] += chars
        else:
            parts.append(w["preamble"] + " " + chars)
    return " ".join(parts)


class PinnedBuffer:
    """nbytes of pinned host memory (pddc_host_alloc) viewed as a numpy uint8 array."""

    def __init__(self, nbytes: int):
        import numpy as np
        p = C.c_void_p()
        check(ddc_lib().pddc_host_alloc(C.byref(p), nbytes))
        self.ptr, self.nbytes = p.value, nbytes
        self.array = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(self.ptr))

    def free(self):
        if getattr(self, "ptr", None):
            self.array = None
            ddc_lib().pddc_host_free(self.ptr)
            self.ptr = None

    __del__ = free


def unpack24_f32(packed_u8, stream=None):
    """torch uint8 CUDA tensor -> float32 [ns, 2] via the HIP kernel."""
    import torch
    ns = packed_u8.numel() // 6
    out = torch.empty((ns, 2), dtype=torch.float32, device=packed_u8.device)
    st = stream if stream is not None else torch.cuda.current_stream(packed_u8.device).cuda_stream
    check(ddc_lib().pddc_unpack24_f32(packed_u8.data_ptr(), ns, out.data_ptr(), st))
    return out


def unpack24_i32(packed_u8, stream=None):
    import torch
    ns = packed_u8.numel() // 6
    out = torch.empty((ns, 2), dtype=torch.int32, device=packed_u8.device)
    st = stream if stream is not None else torch.cuda.current_stream(packed_u8.device).cuda_stream
    check(ddc_lib().pddc_unpack24_i32(packed_u8.data_ptr(), ns, out.data_ptr(), st))
    return out


def pack24_f32(x_f32, stream=None):
    """torch float32 CUDA tensor [ns, 2] -> uint8 wire bytes [6*ns] via the HIP kernel."""
    import torch
    ns = x_f32.numel() // 2
    out = torch.empty(6 * ns + 16, dtype=torch.uint8, device=x_f32.device)
    st = stream if stream is not None else torch.cuda.current_stream(x_f32.device).cuda_stream
    check(ddc_lib().pddc_pack24_f32(x_f32.data_ptr(), ns, out.data_ptr(), st))
    return out[:6 * ns]


def measure_copy(d_dst: int, d_src: int, nbytes: int, iters: int = 20, stream: int = 0) -> float:
    """Average milliseconds of a device-to-device copy of nbytes (pddc_measure_copy)."""
    ms = C.c_float(0)
    check(ddc_lib().pddc_measure_copy(d_dst, d_src, nbytes, iters, stream, C.byref(ms)))
    return float(ms.value)


def synth_lcg(nbytes: int, seed: int = 12345, byte_offset: int = 0, device="cuda:0", stream=None):
    import torch
    out = torch.empty(nbytes, dtype=torch.uint8, device=device)
    st = stream if stream is not None else torch.cuda.current_stream(out.device).cuda_stream
    check(ddc_lib().pddc_synth_lcg(out.data_ptr(), nbytes, seed & 0xFFFFFFFF, byte_offset, st))
    return out


# --------------------------------------------------------------------------
# drop-in perseus_* API (include/perseus-sdr.h, include/perseus-amd-ext.h)
# --------------------------------------------------------------------------
PERSEUS_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p)


class EepromProdId(C.Structure):
    _pack_ = 1
    _fields_ = [("sn", C.c_uint16), ("prodcode", C.c_uint16), ("hwrel", C.c_uint8),
                ("hwver", C.c_uint8), ("signature", C.c_uint8 * 6)]


class AmdConfig(C.Structure):
    _fields_ = [("mode", C.c_int), ("source", C.c_int), ("lcg_seed", C.c_uint32),
                ("file_path", C.c_char_p), ("pace", C.c_int), ("gpu_device", C.c_int),
                ("batch_samples", C.c_uint32), ("drop_every", C.c_int), ("max_buffers", C.c_uint64),
                ("ep_packet_size", C.c_int), ("cpu_source", C.c_int), ("fault_script", C.c_char_p)]


class AmdStats(C.Structure):
    _fields_ = [("delivered", C.c_uint64), ("dropped", C.c_uint64), ("timeouts", C.c_uint64),
                ("dead_transfers", C.c_uint64), ("transfers", C.c_uint64), ("bytes_received", C.c_uint64),
                ("adc_samples", C.c_uint64), ("batches", C.c_uint64), ("gpu_device", C.c_int),
                ("gpu_source", C.c_int), ("peak_receivers_in_flight", C.c_int), ("ganged_batches", C.c_uint64),
                ("buffers_in_place", C.c_uint64), ("buffers_gathered", C.c_uint64)]


_sdr = None


def sdr_lib() -> C.CDLL:
    """Load libperseus-sdr.so (the perseus_* API); raises if not built."""
    global _sdr
    if _sdr is not None:
        return _sdr
    if not os.path.exists(SDR_LIB):
        raise FileNotFoundError(f"{SDR_LIB} is missing: run __graft_entry__.build()")
    ddc_lib()                      # same HIP runtime ordering as above
    L = C.CDLL(SDR_LIB)
    vp = C.c_void_p
    L.perseus_set_debug.argtypes = [C.c_int]
    L.perseus_set_debug.restype = None
    L.perseus_init.restype = C.c_int
    L.perseus_exit.restype = C.c_int
    L.perseus_open.argtypes = [C.c_int]
    L.perseus_open.restype = vp
    L.perseus_close.argtypes = [vp]
    L.perseus_amd_spectrum_enable.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_uint32]
    L.perseus_amd_spectrum_enable.restype = C.c_int
    L.perseus_amd_spectrum_read.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.c_int]
    L.perseus_amd_spectrum_read.restype = C.c_int
    L.perseus_firmware_download.argtypes = [vp, C.c_char_p]
    L.perseus_get_product_id.argtypes = [vp, C.POINTER(EepromProdId)]
    L.perseus_set_attenuator.argtypes = [vp, C.c_uint8]
    L.perseus_set_attenuator_in_db.argtypes = [vp, C.c_int]
    L.perseus_get_attenuator_values.argtypes = [vp, C.POINTER(C.c_int), C.c_uint]
    L.perseus_set_attenuator_n.argtypes = [vp, C.c_int]
    L.perseus_set_adc.argtypes = [vp, C.c_int, C.c_int]
    L.perseus_set_ddc_center_freq.argtypes = [vp, C.c_double, C.c_int]
    L.perseus_start_async_input.argtypes = [vp, C.c_uint32, PERSEUS_CALLBACK, vp]
    L.perseus_stop_async_input.argtypes = [vp]
    L.perseus_set_sampling_rate.argtypes = [vp, C.c_int]
    L.perseus_set_sampling_rate_n.argtypes = [vp, C.c_uint]
    L.perseus_get_sampling_rates.argtypes = [vp, C.POINTER(C.c_int), C.c_uint]
    L.perseus_is_preserie.argtypes = [vp, C.POINTER(C.c_int)]
    L.perseus_errorstr.restype = C.c_char_p
    L.perseus_amd_get_config.argtypes = [vp, C.POINTER(AmdConfig)]
    L.perseus_amd_set_config.argtypes = [vp, C.POINTER(AmdConfig)]
    L.perseus_amd_get_freg.argtypes = [vp]
    L.perseus_amd_get_freg.restype = C.c_uint32
    L.perseus_amd_get_sampling_rate.argtypes = [vp]
    L.perseus_amd_get_frontendctl.argtypes = [vp]
    L.perseus_amd_get_sioctl.argtypes = [vp]
    L.perseus_amd_buffers_delivered.argtypes = [vp]
    L.perseus_amd_buffers_delivered.restype = C.c_uint64
    L.perseus_amd_buffers_dropped.argtypes = [vp]
    L.perseus_amd_buffers_dropped.restype = C.c_uint64
    L.perseus_amd_source_running.argtypes = [vp]
    L.perseus_amd_get_stats.argtypes = [vp, C.POINTER(AmdStats)]
    L.perseus_amd_get_retune_log.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_int]
    L.perseus_amd_get_plan.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                       C.POINTER(C.POINTER(C.c_float))]
    L.perseus_amd_get_plan_interp.argtypes = [vp, C.POINTER(C.c_int)]
    L.perseus_amd_get_plan.restype = C.c_int
    L.perseus_amd_get_plan_interp.restype = C.c_int
    L.perseus_amd_plan_for_rate.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(C.POINTER(C.c_float))]
    L.perseus_amd_plan_for_rate.restype = C.c_int
    L.perseus_amd_effective_batch.argtypes = [vp]
    L.perseus_amd_effective_batch.restype = C.c_uint32
    L.perseus_amd_set_batch.argtypes = [vp, C.c_uint32]
    L.perseus_amd_set_batch.restype = C.c_int
    _sdr = L
    return L


def api_plan(rate: int):
    """The decimation plan the drop-in API builds for perseus_set_sampling_rate(rate) (perseus-sdr.c:776-892 selects the
    rate; the plan and its taps are this library's): [(decim, taps float32, interp)].  perseus_amd_plan_for_rate: no
    descriptor, no perseus_init / perseus_exit -- receivers the process has open are left alone."""
    import numpy as np
    L = sdr_lib()
    dec, nt, it = (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)()
    n = L.perseus_amd_plan_for_rate(int(rate), None, dec, nt, it, None)
    if n < 0:
        raise RuntimeError(f"perseus_amd_plan_for_rate({rate}): {n}")
    taps = [np.zeros(nt[i], np.float32) for i in range(n)]
    arr = (C.POINTER(C.c_float) * 4)(*([t.ctypes.data_as(C.POINTER(C.c_float)) for t in taps] + [None] * (4 - n)))
    L.perseus_amd_plan_for_rate(int(rate), None, dec, nt, it, arr)
    return [(int(dec[i]), taps[i], int(it[i])) for i in range(n)]
