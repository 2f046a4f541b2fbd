"""ctypes binding of liblorahip.so (include/lorahip.h). No fallbacks: if the shared library
is missing or a call fails, this raises -- there is no CPU path in the product."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# LORAHIP_LIB: another build of the same library (A/B measurements of kernel changes inside one GPU session, tools/gpu_ab.sh)
LIB_PATH = os.environ.get("LORAHIP_LIB") or os.path.join(HERE, "liblorahip.so")

OK = 0
SF_MIN, SF_MAX = 6, 12
FINE_STEPS = 128
CHIRP_UP, CHIRP_DOWN, CHIRP_NONE = 0, 1, 2
IQ_CF32, IQ_SC16, IQ_SC8 = 0, 1, 2         # LORAHIP_IQ_*: the sample formats the receive front ends read and the synthesisers write

_f32p = C.POINTER(C.c_float)


class LoraHipError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        lib = load()
        msg = lib.lorahip_strerror(code).decode()
        detail = lib.lorahip_last_error().decode()
        super().__init__("%s failed: %s (%d)%s" % (where, msg, code, (": " + detail) if detail and code == -3 else ""))


class Batch(C.Structure):
    """struct lorahip_batch"""
    _fields_ = [("struct_size", C.c_size_t),
                ("iq", C.c_void_p), ("n_windows", C.c_size_t), ("offsets", C.c_void_p),
                ("window_stride", C.c_size_t), ("chirp_sel", C.c_void_p), ("chirp_sel_all", C.c_int32),
                ("fine_idx0", C.c_void_p), ("fine_err", C.c_void_p),
                ("sym", C.c_void_p), ("power", C.c_void_p), ("power_avg", C.c_void_p), ("f_index", C.c_void_p),
                ("fine_idx_out", C.c_void_p), ("fft_out", C.c_void_p), ("dec_out", C.c_void_p)]


class DecoderCfg(C.Structure):
    _fields_ = [("struct_size", C.c_size_t)] + [(n, C.c_int32) for n in ("sf", "ppm", "rdd", "crcc", "interleaving", "error_check",
                                                                          "explicit_hdr", "hdr", "data_length")]


RDD_FROM_HEADER = -1      # LORAHIP_RDD_FROM_HEADER: DecoderCfg.rdd, the coding rate each packet's explicit header names


class PacketInfo(C.Structure):
    """struct lorahip_packet_info (32 bytes): the header report of one packet"""
    _fields_ = [(n, C.c_int32) for n in ("length", "rdd", "crc", "hdr_residue", "fec_error", "need_syms")] + [("reserved", C.c_int32 * 2)]


class EncoderCfg(C.Structure):
    """struct lorahip_encoder_cfg"""
    _fields_ = [("struct_size", C.c_size_t)] + [(n, C.c_int32) for n in ("sf", "ppm", "rdd", "explicit_hdr", "crc", "whitening")]


class DemodPorts(C.Structure):
    """struct lorahip_demod_ports"""
    _fields_ = [("struct_size", C.c_size_t), ("fft_dev", C.c_void_p), ("fft_cap_frames", C.c_size_t), ("dec_dev", C.c_void_p),
                ("dec_cap_samples", C.c_size_t), ("raw_dev", C.c_void_p), ("raw_cap_samples", C.c_size_t),
                ("host_buffers", C.c_int32), ("reserved", C.c_int32)]


class ResamplerTiling(C.Structure):
    """struct lorahip_resampler_tiling"""
    _fields_ = [(n, C.c_size_t) for n in ("ns", "rg", "pb", "n_phase_blocks", "ti", "qp", "waves", "lds_bytes", "t", "up_reduced", "down_reduced")]


class DecodeTiling(C.Structure):
    """struct lorahip_decode_tiling"""
    _fields_ = [("struct_size", C.c_size_t)] + [(n, C.c_int32) for n in ("lanes_per_packet", "sym_cap", "cw_cap", "lds_slice_bytes",
                                                                          "packets_per_workgroup", "reserved")]


class SoftTiling(C.Structure):
    """struct lorahip_soft_tiling"""
    _fields_ = [("struct_size", C.c_size_t)] + [(n, C.c_int32) for n in ("runs_per_wavefront", "waves_per_workgroup", "workgroups", "reserved")]


class PacketRows(C.Structure):
    """struct lorahip_packet_rows"""
    _fields_ = [("struct_size", C.c_size_t), ("syms_dev", C.c_void_p), ("sym_stride", C.c_size_t), ("nsyms_dev", C.c_void_p),
                ("channel_dev", C.c_void_p), ("cap_packets", C.c_size_t), ("async_", C.c_int32), ("reserved", C.c_int32)]


class PacketRowsInfo(PacketRows):
    """struct lorahip_packet_rows with its last member, info_dev (PacketRows is the previous struct_size, which the library still takes: no info)"""
    _fields_ = [("info_dev", C.c_void_p)]


class SignalRows(C.Structure):
    """struct lorahip_signal_rows"""
    _fields_ = [("struct_size", C.c_size_t), ("channel", C.c_void_p), ("error", C.c_void_p), ("power", C.c_void_p), ("snr", C.c_void_p), ("cap", C.c_size_t)]


class SignalRowsPos(SignalRows):
    """struct lorahip_signal_rows with its last member, pos (SignalRows is the previous struct_size: no positions)"""
    _fields_ = [("pos", C.c_void_p)]


class RxInfo(C.Structure):
    """struct lorahip_rx_info (32 bytes): when a packet arrived, in samples of its channel's stream. P of them are a (P, 4) int64
    array, which is how the Python layer hands them out; RxInfo.COLUMNS names the columns and RxInfo.view(a) gives a numpy array of
    that shape the fields by name (a["end_pos"], ...)."""
    _fields_ = [(n, C.c_int64) for n in ("end_pos", "data_pos", "sync_pos", "freq_error")]
    COLUMNS = ("end_pos", "data_pos", "sync_pos", "freq_error")
    END_POS, DATA_POS, SYNC_POS, FREQ_ERROR = range(4)

    @staticmethod
    def view(a):
        import numpy as np
        a = np.ascontiguousarray(a, np.int64).reshape(-1, 4)
        return a.view(np.dtype([(n, np.int64) for n in RxInfo.COLUMNS])).reshape(-1)


class WorkResult(C.Structure):
    """struct lorahip_work_result"""
    _fields_ = [("consumed", C.c_int64), ("state_before", C.c_int32), ("value", C.c_int32),
                ("power", C.c_float), ("power_avg", C.c_float), ("snr", C.c_float), ("f_index", C.c_float),
                ("worked", C.c_int32), ("packet_len", C.c_int32), ("signals", C.c_int32),
                ("sig_error", C.c_int32), ("sig_power", C.c_float), ("sig_snr", C.c_float),
                ("fine_idx_before", C.c_int32), ("fine_idx_after", C.c_int32), ("fine_err_before", C.c_float), ("reserved", C.c_int32)]


# every symbol include/lorahip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "lorahip_strerror": (C.c_char_p, [C.c_int]),
    "lorahip_last_error": (C.c_char_p, []),
    "lorahip_version": (C.c_int, []),
    "lorahip_selfcheck": (C.c_int, []),
    "lorahip_device_count": (C.c_int, []),
    "lorahip_host_tables": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lorahip_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "lorahip_destroy": (None, [C.c_void_p]),
    "lorahip_sf": (C.c_int, [C.c_void_p]),
    "lorahip_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lorahip_synchronize": (C.c_int, [C.c_void_p]),
    "lorahip_reset_stream": (C.c_int, [C.c_void_p]),
    "lorahip_demod_reset_stream": (C.c_int, [C.c_void_p]),
    "lorahip_set_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "lorahip_set_fine_gather": (C.c_int, [C.c_void_p, C.c_int]),
    "lorahip_fine_split_active": (C.c_int, [C.c_void_p]),
    "lorahip_fine_split_selftest": (C.c_int, [C.c_int]),
    "lorahip_fine_indices_host": (C.c_int, [C.c_int, C.c_int32, C.c_float, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lorahip_demod_set_fine_gather": (C.c_int, [C.c_void_p, C.c_int]),
    "lorahip_demod_set_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "lorahip_demod_set_stream_grid": (C.c_int, [C.c_void_p, C.c_int]),
    "lorahip_demod_set_record_capacity": (C.c_int, [C.c_void_p, C.c_size_t]),
    "lorahip_demod_set_stream_lanes": (C.c_int, [C.c_void_p, C.c_int]),
    "lorahip_demod_run_host_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "lorahip_demod_stream_lanes": (C.c_int, [C.c_void_p]),
    "lorahip_demod_stream_wait": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lorahip_demod_stream_follow": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lorahip_detect_batch": (C.c_int, [C.c_void_p, C.POINTER(Batch)]),
    "lorahip_detect_batch_host": (C.c_int, [C.c_void_p, C.POINTER(Batch)]),
    "lorahip_mixed_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t]),
    "lorahip_mixed_destroy": (None, [C.c_void_p]),
    "lorahip_mixed_num_buckets": (C.c_size_t, [C.c_void_p]),
    "lorahip_mixed_bucket": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lorahip_mixed_context": (C.c_void_p, [C.c_void_p, C.c_size_t]),
    "lorahip_mixed_rows": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lorahip_mixed_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "lorahip_mixed_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lorahip_mixed_synchronize": (C.c_int, [C.c_void_p]),
    "lorahip_shard_plan": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "lorahip_mixed_create_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lorahip_mixed_num_devices": (C.c_size_t, [C.c_void_p]),
    "lorahip_mixed_device": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "lorahip_mixed_shard": (C.c_void_p, [C.c_void_p, C.c_size_t]),
    "lorahip_mixed_shard_of": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lorahip_mixed_detect_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lorahip_host_alloc": (C.c_void_p, [C.c_size_t]),
    "lorahip_host_free": (None, [C.c_void_p]),
    "lorahip_timer_start": (C.c_int, [C.c_void_p]),
    "lorahip_timer_stop": (C.c_int, [C.c_void_p, _f32p]),
    "lorahip_detector_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_size_t]),
    "lorahip_detector_destroy": (None, [C.c_void_p]),
    "lorahip_detector_feed": (C.c_int, [C.c_void_p, C.c_size_t, C.c_float, C.c_float]),
    "lorahip_detector_detect": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), _f32p, _f32p, _f32p, C.c_void_p]),
    "lorahip_demod_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_size_t]),
    "lorahip_demod_destroy": (None, [C.c_void_p]),
    "lorahip_demod_create_mixed": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lorahip_demod_num_channels": (C.c_size_t, [C.c_void_p]),
    "lorahip_demod_num_parts": (C.c_size_t, [C.c_void_p]),
    "lorahip_demod_part": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "lorahip_demod_part_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "lorahip_demod_part_handle": (C.c_void_p, [C.c_void_p, C.c_size_t]),
    "lorahip_demod_run_device_segments_multi": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "lorahip_demod_run_device_append": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int64)]),
    "lorahip_demod_rewind": (C.c_int, [C.c_void_p]),
    "lorahip_demod_receive": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(PacketRows), C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "lorahip_demod_receive_flush": (C.c_int, [C.c_void_p, C.POINTER(PacketRows), C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "lorahip_demod_receive_signal_rows": (C.c_int, [C.c_void_p, C.POINTER(SignalRows)]),
    "lorahip_demod_receive_num_signals": (C.c_size_t, [C.c_void_p]),
    "lorahip_demod_resident_active": (C.c_int, [C.c_void_p]),
    "lorahip_demod_receive_steps": (C.c_size_t, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_size_t]),
    "lorahip_demod_set_signals": (C.c_int, [C.c_void_p, C.c_int]),
    "lorahip_demod_num_signals": (C.c_size_t, [C.c_void_p]),
    "lorahip_demod_get_signals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "lorahip_demod_set_sync": (C.c_int, [C.c_void_p, C.c_ubyte]),
    "lorahip_demod_set_threshold": (C.c_int, [C.c_void_p, C.c_double]),
    "lorahip_demod_set_mtu": (C.c_int, [C.c_void_p, C.c_size_t]),
    "lorahip_mod_frame_len": (C.c_size_t, [C.c_int, C.c_size_t, C.c_size_t]),
    "lorahip_mod_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_ubyte, C.c_float, C.c_size_t]),
    "lorahip_add_awgn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_uint64]),
    "lorahip_decode_packets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_void_p]),
    "lorahip_decode_packets_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_void_p]),
    "lorahip_decode_packets_cfgs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lorahip_decode_packets_cfgs_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "lorahip_decode_packets_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lorahip_decode_packets_info_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lorahip_soft_symbols": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                      C.c_void_p]),
    "lorahip_soft_plan": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "lorahip_decode_packets_soft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lorahip_decode_packets_soft_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lorahip_decode_plan": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "lorahip_decode_max_symbols": (C.c_int, []),
    "lorahip_decode_max_data_length": (C.c_int, []),
    "lorahip_encode_num_symbols": (C.c_long, [C.c_void_p, C.c_size_t]),
    "lorahip_encode_max_bytes": (C.c_int, []),
    "lorahip_encode_packets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lorahip_encode_packets_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lorahip_mod_frames_var": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_ubyte,
                                        C.c_float, C.c_size_t]),
    "lorahip_encode_packets_cfgs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lorahip_encode_packets_cfgs_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lorahip_mod_body_len": (C.c_size_t, [C.c_int, C.c_size_t]),
    "lorahip_mod_frames_sched": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_ubyte, C.c_float, C.c_int, C.c_void_p]),
    "lorahip_channelizer_phase_inc": (C.c_uint64, [C.c_double]),
    "lorahip_channelizer_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lorahip_channelizer_destroy": (None, [C.c_void_p]),
    "lorahip_channelizer_reset": (C.c_int, [C.c_void_p]),
    "lorahip_channelizer_out_count": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "lorahip_channelizer_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lorahip_channelizer_run_captures": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lorahip_iq_sample_bytes": (C.c_size_t, [C.c_int]),
    "lorahip_channelizer_run_iq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lorahip_channelizer_run_captures_iq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                     C.POINTER(C.c_size_t)]),
    "lorahip_synthesizer_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lorahip_synthesizer_destroy": (None, [C.c_void_p]),
    "lorahip_synthesizer_reset": (C.c_int, [C.c_void_p]),
    "lorahip_synthesizer_out_count": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "lorahip_synthesizer_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]),
    "lorahip_pfb_check": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    "lorahip_pfb_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lorahip_pfb_check_radix5": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    "lorahip_pfb_create_radix5": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lorahip_pfb_destroy": (None, [C.c_void_p]),
    "lorahip_pfb_reset": (C.c_int, [C.c_void_p]),
    "lorahip_pfb_out_count": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "lorahip_pfb_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lorahip_pfb_run_iq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lorahip_psb_check": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    "lorahip_psb_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lorahip_psb_check_radix5": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    "lorahip_psb_create_radix5": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lorahip_psb_destroy": (None, [C.c_void_p]),
    "lorahip_psb_reset": (C.c_int, [C.c_void_p]),
    "lorahip_psb_out_count": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "lorahip_psb_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]),
    "lorahip_synthesizer_run_iq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_size_t)]),
    "lorahip_psb_run_iq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_size_t)]),
    "lorahip_synthesizer_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "lorahip_psb_clipped": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "lorahip_resampler_check": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    "lorahip_resampler_plan": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p]),
    "lorahip_resampler_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lorahip_resampler_destroy": (None, [C.c_void_p]),
    "lorahip_resampler_reset": (C.c_int, [C.c_void_p]),
    "lorahip_resampler_reset_at": (C.c_int, [C.c_void_p, C.c_uint64]),
    "lorahip_resampler_out_count": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "lorahip_resampler_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lorahip_resampler_run_iq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lorahip_demod_activate": (C.c_int, [C.c_void_p]),
    "lorahip_demod_set_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "lorahip_demod_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lorahip_demod_packets_to_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lorahip_demod_packets_to_device_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lorahip_demod_get_packets_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "lorahip_demod_get_signals_pos": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "lorahip_demod_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "lorahip_demod_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64)]),
    "lorahip_demod_run_device_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "lorahip_demod_num_packets": (C.c_size_t, [C.c_void_p]),
    "lorahip_demod_get_packet": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_size_t), C.c_void_p, C.c_size_t]),
    "lorahip_demod_num_packet_symbols": (C.c_size_t, [C.c_void_p]),
    "lorahip_demod_get_packets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lorahip_demod_clear_packets": (None, [C.c_void_p]),
    "lorahip_demod_consumed": (C.c_int64, [C.c_void_p, C.c_size_t]),
    "lorahip_demod_consumed_all": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "lorahip_demod_work_calls": (C.c_int64, [C.c_void_p]),
    "lorahip_demod_kernel_ms": (C.c_double, [C.c_void_p]),
    "lorahip_demod_last_launches": (C.c_int, [C.c_void_p]),
    "lorahip_demod_near_threshold": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lorahip_demod_set_trace": (C.c_int, [C.c_void_p, C.c_int]),
    "lorahip_demod_set_ports": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lorahip_demod_port_counts": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lorahip_demod_get_labels": (C.c_int, [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lorahip_demod_trace_len": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "lorahip_demod_get_trace": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(WorkResult), C.c_size_t]),
    "lorahip_membw_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    "lorahip_synth_symbols": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float,
                                        C.c_uint64]),
}

_lib = None


def load():
    """Load liblorahip.so (once). Raises OSError with a build hint if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("%s not found: build it with `python -m lora_sdr_amd.build` "
                      "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    try:
        # bring in torch's HIP runtime first when torch is around, so that one libamdhip64 is shared
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C ABI itself
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)     # AttributeError here = header/library mismatch
        except AttributeError:
            if os.environ.get("LORAHIP_LIB"):
                continue                # an older build under A/B measurement lacks newer entry points: calling one still fails
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code, where):
    if code != OK:
        raise LoraHipError(code, where)
