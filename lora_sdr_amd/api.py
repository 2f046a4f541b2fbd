"""Host-side mirror of the reference's operator interface for the demod hot path, on top of
the C ABI (include/lorahip.h). Names and argument meaning follow the reference:

  LoRaDetector(N).feed(i, samp) / .detect()      LoRaDetector.hpp:8-72
  LoRaDemod(sf).setSync/.setThreshold/.setMTU    LoRaDemod.cpp:119-137   (factory /lora/lora_demod)
  LoRaDemod.activate() / .work(...)              LoRaDemod.cpp:139-327
  Context(sf).detect_batch(...)                  the batched form of LoRaDemod.cpp:157-172

torch is used for device memory and streams only.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Batch, DecoderCfg, EncoderCfg, WorkResult, check, load, CHIRP_UP, CHIRP_DOWN, CHIRP_NONE  # noqa: F401


# lorahip_work_result as a numpy record (include/lorahip.h)
WORK_RESULT_DTYPE = np.dtype([("consumed", np.int64), ("state_before", np.int32), ("value", np.int32), ("power", np.float32),
                              ("power_avg", np.float32), ("snr", np.float32), ("f_index", np.float32), ("worked", np.int32),
                              ("packet_len", np.int32), ("signals", np.int32), ("sig_error", np.int32), ("sig_power", np.float32),
                              ("sig_snr", np.float32), ("fine_idx_before", np.int32), ("fine_idx_after", np.int32),
                              ("fine_err_before", np.float32), ("reserved", np.int32)])


def host_tables(sf, fine=True):
    """(up, down, fine, twiddle) exactly as the reference builds them -- pure host code."""
    lib = load()
    N = 1 << sf
    up = np.empty(N, np.complex64)
    down = np.empty(N, np.complex64)
    fi = np.empty(N * _lib.FINE_STEPS, np.complex64) if fine else None
    tw = np.empty(N, np.complex64)
    check(lib.lorahip_host_tables(sf, up.ctypes.data, down.ctypes.data, fi.ctypes.data if fine else None,
                                  tw.ctypes.data), "lorahip_host_tables")
    return up, down, fi, tw


def device_count():
    return load().lorahip_device_count()


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _dptr(t, dtype=None):
    """device pointer of a torch tensor (must be contiguous, on a HIP device)"""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("expected a device tensor")
    if not t.is_contiguous():
        raise ValueError("expected a contiguous tensor")
    if dtype is not None and t.dtype != dtype:
        raise ValueError("expected dtype %s, got %s" % (dtype, t.dtype))
    return t.data_ptr()


class _Handle:
    """One object of the C library: the library `_lib`, the handle `_h`, and close() -- at garbage collection too, and harmless when
    repeated -- through the destroy entry point the class names in `_destroy`."""

    _destroy = None

    def __init__(self):
        self._lib = load()
        self._h = C.c_void_p()

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(self._lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    __del__ = close


class Context(_Handle):
    """One (device, SF) batch context: chirp / fine-tune / twiddle tables resident in HBM."""

    _destroy = "lorahip_destroy"

    def __init__(self, sf, device=0):
        super().__init__()
        check(self._lib.lorahip_create(C.byref(self._h), int(device), int(sf)), "lorahip_create")
        self.sf = int(sf)
        self.N = 1 << self.sf
        self.device = int(device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, stream_handle):
        """stream_handle: integer hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); 0/None is
        HIP's null stream, which is torch's default stream"""
        check(self._lib.lorahip_set_stream(self._h, C.c_void_p(stream_handle or 0)), "lorahip_set_stream")

    def use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def set_variant(self, v):
        check(self._lib.lorahip_set_variant(self._h, int(v)), "lorahip_set_variant")

    def synchronize(self):
        check(self._lib.lorahip_synchronize(self._h), "lorahip_synchronize")

    def set_fine_gather(self, on):
        """A/B switch: read the fine-tune table in HBM instead of evaluating it from the split tables (include/lorahip.h)"""
        check(self._lib.lorahip_set_fine_gather(self._h, int(bool(on))), "lorahip_set_fine_gather")

    def fine_split_active(self):
        return bool(self._lib.lorahip_fine_split_active(self._h))

    def timer_start(self):
        check(self._lib.lorahip_timer_start(self._h), "lorahip_timer_start")

    def timer_stop(self):
        ms = C.c_float()
        check(self._lib.lorahip_timer_stop(self._h, C.byref(ms)), "lorahip_timer_stop")
        return ms.value

    # ------------------------------------------------------------------
    def detect_batch_raw(self, batch):
        """Launch with a prepared struct lorahip_batch of DEVICE pointers (asynchronous)."""
        check(self._lib.lorahip_detect_batch(self._h, C.byref(batch)), "lorahip_detect_batch")

    def make_batch(self, iq, n_windows, sym, power, power_avg, f_index, offsets=None, window_stride=0,
                   chirp_sel=None, chirp_sel_all=CHIRP_UP, fine_idx0=None, fine_err=None, fine_idx_out=None,
                   fft_out=None, dec_out=None):
        """Build a struct lorahip_batch from torch device tensors (kept alive by the caller)."""
        import torch
        b = Batch()
        b.struct_size = C.sizeof(Batch)
        b.iq = _dptr(iq)
        b.n_windows = int(n_windows)
        b.offsets = _dptr(offsets, torch.int64)
        b.window_stride = int(window_stride)
        b.chirp_sel = _dptr(chirp_sel, torch.int32)
        b.chirp_sel_all = int(chirp_sel_all)
        b.fine_idx0 = _dptr(fine_idx0, torch.int32)
        b.fine_err = _dptr(fine_err, torch.float32)
        b.sym = _dptr(sym)
        b.power = _dptr(power, torch.float32)
        b.power_avg = _dptr(power_avg, torch.float32)
        b.f_index = _dptr(f_index, torch.float32)
        b.fine_idx_out = _dptr(fine_idx_out, torch.int32)
        b.fft_out = _dptr(fft_out)
        b.dec_out = _dptr(dec_out)
        return b

    def detect_batch(self, iq, n_windows=None, offsets=None, window_stride=0, chirp_sel=None,
                     chirp_sel_all=CHIRP_UP, fine_idx0=None, fine_err=None, want_fft=False, want_dec=False,
                     want_fine_idx=False):
        """Demodulate a batch of independent windows.

        iq: torch complex64 device tensor (flat stream) or numpy complex64 array (host; staged
        through the context). Returns a dict of arrays of the same kind as the input:
        sym (uint16 as int16-viewed tensor for torch), power, powerAvg, fIndex [, fineIdxOut, fft, dec].
        """
        if _is_torch(iq):
            return self._detect_torch(iq, n_windows, offsets, window_stride, chirp_sel, chirp_sel_all,
                                      fine_idx0, fine_err, want_fft, want_dec, want_fine_idx)
        return self._detect_numpy(iq, n_windows, offsets, window_stride, chirp_sel, chirp_sel_all,
                                  fine_idx0, fine_err, want_fft, want_dec, want_fine_idx)

    def _count(self, n_samples, n_windows, offsets, window_stride):
        if offsets is not None:
            return int(offsets.shape[0])
        if n_windows is not None:
            return int(n_windows)
        stride = window_stride or self.N
        return 0 if n_samples < self.N else (n_samples - self.N) // stride + 1

    def _detect_torch(self, iq, n_windows, offsets, window_stride, chirp_sel, chirp_sel_all, fine_idx0, fine_err,
                      want_fft, want_dec, want_fine_idx):
        import torch
        iq = iq.reshape(-1)
        dev = iq.device
        W = self._count(iq.numel(), n_windows, offsets, window_stride)
        out = dict(sym=torch.empty(W, dtype=torch.int16, device=dev),       # uint16 payload
                   power=torch.empty(W, dtype=torch.float32, device=dev),
                   powerAvg=torch.empty(W, dtype=torch.float32, device=dev),
                   fIndex=torch.empty(W, dtype=torch.float32, device=dev))
        if want_fine_idx:
            out["fineIdxOut"] = torch.empty(W, dtype=torch.int32, device=dev)
        if want_fft:
            out["fft"] = torch.empty((W, self.N), dtype=torch.complex64, device=dev)
        if want_dec:
            out["dec"] = torch.empty((W, self.N), dtype=torch.complex64, device=dev)
        b = self.make_batch(iq, W, out["sym"], out["power"], out["powerAvg"], out["fIndex"], offsets=offsets,
                            window_stride=window_stride, chirp_sel=chirp_sel, chirp_sel_all=chirp_sel_all,
                            fine_idx0=fine_idx0, fine_err=fine_err, fine_idx_out=out.get("fineIdxOut"),
                            fft_out=out.get("fft"), dec_out=out.get("dec"))
        self.use_torch_stream()
        self.detect_batch_raw(b)
        return out

    def _detect_numpy(self, iq, n_windows, offsets, window_stride, chirp_sel, chirp_sel_all, fine_idx0, fine_err,
                      want_fft, want_dec, want_fine_idx):
        iq = np.ascontiguousarray(iq, np.complex64).reshape(-1)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, np.int64)
        W = self._count(iq.size, n_windows, offsets, window_stride)
        cs = None if chirp_sel is None else np.ascontiguousarray(np.broadcast_to(chirp_sel, (W,)), np.int32)
        i0 = None if fine_idx0 is None else np.ascontiguousarray(np.broadcast_to(fine_idx0, (W,)), np.int32)
        fe = None if fine_err is None else np.ascontiguousarray(np.broadcast_to(fine_err, (W,)), np.float32)
        out = dict(sym=np.empty(W, np.uint16), power=np.empty(W, np.float32), powerAvg=np.empty(W, np.float32),
                   fIndex=np.empty(W, np.float32))
        if want_fine_idx:
            out["fineIdxOut"] = np.empty(W, np.int32)
        if want_fft:
            out["fft"] = np.empty((W, self.N), np.complex64)
        if want_dec:
            out["dec"] = np.empty((W, self.N), np.complex64)
        need = (int(offsets.max()) + self.N) if (offsets is not None and W) else ((W - 1) * (window_stride or self.N) + self.N if W else 0)
        if need > iq.size:
            raise ValueError("iq holds %d samples, the batch reads up to %d" % (iq.size, need))

        def p(a):
            return None if a is None else a.ctypes.data
        b = Batch()
        b.struct_size = C.sizeof(Batch)
        b.iq = p(iq)
        b.n_windows = W
        b.offsets = p(offsets)
        b.window_stride = int(window_stride)
        b.chirp_sel = p(cs)
        b.chirp_sel_all = int(chirp_sel_all)
        b.fine_idx0 = p(i0)
        b.fine_err = p(fe)
        b.sym = p(out["sym"]); b.power = p(out["power"]); b.power_avg = p(out["powerAvg"]); b.f_index = p(out["fIndex"])
        b.fine_idx_out = p(out.get("fineIdxOut"))
        b.fft_out = p(out.get("fft"))
        b.dec_out = p(out.get("dec"))
        check(self._lib.lorahip_detect_batch_host(self._h, C.byref(b)), "lorahip_detect_batch_host")
        return out

    def synth_symbols(self, sym, ampl=1.0, noise_sigma=0.0, seed=0):
        """IQ of len(sym) back-to-back up-chirp symbols generated in HBM -> complex64 device tensor. Symbols are masked to their
        low sf bits (mod_frames does not mask)."""
        import torch
        sym = sym.reshape(-1)
        if sym.dtype not in (torch.int16, torch.uint16):
            raise ValueError("sym must be a 16-bit integer device tensor")
        iq = torch.empty(sym.numel() * self.N, dtype=torch.complex64, device=sym.device)
        self.use_torch_stream()
        check(self._lib.lorahip_synth_symbols(self._h, _dptr(iq), _dptr(sym), sym.numel(), float(ampl),
                                              float(noise_sigma), int(seed) & (2 ** 64 - 1)), "lorahip_synth_symbols")
        return iq

    def soft_symbols(self, iq, first_sample, nsyms, fine_idx0=None, fine_err=None, ppm=0, sym_stride=None, hard=False, out=None):
        """Per-bit log-likelihood ratios of P runs of consecutive symbol windows (lorahip_soft_symbols: the definition is in
        include/lorahip.h). iq: complex64 device tensor (flat stream); first_sample (P,) int64, nsyms (P,) int32, fine_idx0 (P,) int32 or
        None, fine_err (P,) float32 or None -- device tensors. -> llr (P, sym_stride, ppm) float32, zero behind a run's windows; with
        hard=True also sym (P, sym_stride) int16 (uint16 payload), the hard symbol of each window. sym_stride must be given (a default
        would have to read nsyms back): nothing here waits for the device. out: the caller's llr (or (llr, sym) with hard=True) to
        write into instead of new zeroed tensors; entries behind a run's windows are left as they are."""
        import torch
        if sym_stride is None:
            raise ValueError("soft_symbols: sym_stride (windows per row) must be given")
        iq = iq.reshape(-1)
        P, S, W = int(nsyms.numel()), int(sym_stride), int(ppm) or self.sf
        if first_sample.numel() != P or any(x is not None and x.numel() != P for x in (fine_idx0, fine_err)):
            raise ValueError("soft_symbols: one entry per run in first_sample, nsyms, fine_idx0, fine_err")
        if out is not None:                               # the caller's rows: entries behind a run's windows stay as they are
            llr, sym = out if hard else (out, None)
            if tuple(llr.shape) != (P, S, W) or (hard and tuple(sym.shape) != (P, S)) or (hard and sym.dtype not in (torch.int16, torch.uint16)):
                raise ValueError("soft_symbols: out must be llr (P, sym_stride, ppm) float32 [, sym (P, sym_stride) 16-bit]")
        else:
            llr = torch.zeros((P, S, W), dtype=torch.float32, device=iq.device)
            sym = torch.zeros((P, S), dtype=torch.int16, device=iq.device) if hard else None
        self.use_torch_stream()
        check(self._lib.lorahip_soft_symbols(self._h, _dptr(iq, torch.complex64), _dptr(first_sample, torch.int64), _dptr(nsyms, torch.int32),
                                             _dptr(fine_idx0, torch.int32), _dptr(fine_err, torch.float32), P, int(ppm), _dptr(llr, torch.float32), S,
                                             _dptr(sym)), "lorahip_soft_symbols")
        return (llr, sym) if hard else llr

    def soft_plan(self, n_packets):
        """what soft_symbols launches for n_packets runs (lorahip_soft_plan; no device work): a dict with the fields of struct
        lorahip_soft_tiling in include/lorahip.h"""
        t = _lib.SoftTiling(C.sizeof(_lib.SoftTiling))
        check(self._lib.lorahip_soft_plan(self._h, int(n_packets), C.byref(t)), "lorahip_soft_plan")
        return dict((f, int(getattr(t, f))) for f, _ in _lib.SoftTiling._fields_ if f not in ("struct_size", "reserved"))

    # ------------------------------------------------------------------
    def mod_frame_len(self, nsyms, padding=1):
        return int(self._lib.lorahip_mod_frame_len(self.sf, int(nsyms), int(padding)))

    def mod_frames(self, syms, sync=0x12, ampl=1.0, padding=1, frame_stride=None, lead=0, tail=0, nsyms=None):
        """The LoRaMod block (LoRaMod.cpp:109-238) for a batch of packets: syms is a (n_frames, nsyms) 16-bit device
        tensor; returns a (n_frames, lead + frame_stride + tail) complex64 device tensor, zero outside the frames. Symbols are
        used as given (f0 = 2 pi sym / N also for sym >= N, as the block does; synth_symbols masks to sf bits instead).

        nsyms: an optional (n_frames,) int32 device tensor of per-frame symbol counts (the encoder's output), read on the device
        (lorahip_mod_frames_var): frame f is modulated from its first nsyms[f] symbols and continued with zero chirps to the length
        of a frame of syms.shape[1] symbols; a negative or larger count gives an all-zero row."""
        import torch
        if syms.dim() != 2 or syms.dtype not in (torch.int16, torch.uint16):
            raise ValueError("syms must be a (n_frames, nsyms) 16-bit integer device tensor")
        syms = syms.contiguous()
        F, S = int(syms.shape[0]), int(syms.shape[1])
        flen = self.mod_frame_len(S, padding)
        stride = int(frame_stride or flen)
        if stride < flen:
            raise ValueError("frame_stride %d is shorter than the frame (%d samples)" % (stride, flen))
        row = lead + stride + tail
        iq = torch.zeros((F, row), dtype=torch.complex64, device=syms.device)
        self.use_torch_stream()
        base = iq.data_ptr() + 8 * lead
        if nsyms is not None:
            if nsyms.dtype != torch.int32 or nsyms.numel() != F:
                raise ValueError("nsyms must be a (n_frames,) int32 device tensor")
            check(self._lib.lorahip_mod_frames_var(self._h, C.c_void_p(base), row, _dptr(syms), S, _dptr(nsyms.contiguous()), F, S,
                                                   int(sync) & 0xff, float(ampl), int(padding)), "lorahip_mod_frames_var")
            return iq
        check(self._lib.lorahip_mod_frames(self._h, C.c_void_p(base), row, _dptr(syms), F, S, int(sync) & 0xff, float(ampl),
                                           int(padding)), "lorahip_mod_frames")
        return iq

    def mod_frames_sched(self, syms, nsyms, sf, row, start, out, ampl=1.0, ampl_of=None, sync=0x12, lanes=0):
        """Frames of different SF into channel rows (lorahip_mod_frames_sched): frame f is the body -- preamble, sync, down-chirps and the
        first nsyms[f] data chirps, lorahip_mod_body_len(sf[f], nsyms[f]) samples -- of the frame mod_frames makes at SF sf[f], written at
        out[row[f], start[f]:start[f] + body]. Nothing else of `out` is touched; frames must not overlap.

        syms: (F, stride) 16-bit, nsyms / sf / row: (F,) int32, start: (F,) int64, ampl_of: (F,) float32 or None (`ampl` for every frame) --
        device tensors; out: a (n_rows, row_len) complex64 device tensor whose rows are contiguous (a row stride above row_len is fine).
        lanes: 0 (by the frame count), 4, 16 or 64 lanes of a wavefront per frame. The context's own SF plays no part.
        Returns status, (F,) int32: 0 written, -1 no usable symbol count, -2 the body does not fit the row, -3 no such SF or row."""
        import torch
        if syms.dim() != 2 or syms.dtype not in (torch.int16, torch.uint16):
            raise ValueError("syms must be a (n_frames, stride) 16-bit integer device tensor")
        F, S = int(syms.shape[0]), int(syms.shape[1])
        for name, v, dt in (("nsyms", nsyms, torch.int32), ("sf", sf, torch.int32), ("row", row, torch.int32), ("start", start, torch.int64)):
            if v.dtype != dt or v.numel() != F:
                raise ValueError("%s must be a (n_frames,) %s device tensor" % (name, str(dt).replace("torch.", "")))
        if ampl_of is not None and (ampl_of.dtype != torch.float32 or ampl_of.numel() != F):
            raise ValueError("ampl_of must be a (n_frames,) float32 device tensor")
        if out.dim() != 2 or out.dtype != torch.complex64 or (out.shape[1] > 1 and out.stride(1) != 1) or \
                (out.shape[0] > 1 and out.stride(0) < out.shape[1]) or not out.is_cuda:
            raise ValueError("out must be a (n_rows, row_len) complex64 device tensor with contiguous rows")
        syms, nsyms, sf, row, start = syms.contiguous(), nsyms.contiguous(), sf.contiguous(), row.contiguous(), start.contiguous()
        ampl_of = None if ampl_of is None else ampl_of.contiguous()
        status = torch.empty(F, dtype=torch.int32, device=syms.device)
        self.use_torch_stream()
        row_stride = int(out.stride(0)) if out.shape[0] > 1 else int(out.shape[1])
        check(self._lib.lorahip_mod_frames_sched(self._h, C.c_void_p(out.data_ptr()), int(out.shape[0]), row_stride, int(out.shape[1]), _dptr(syms), S,
                                                 _dptr(nsyms), _dptr(sf), _dptr(row), _dptr(start), None if ampl_of is None else _dptr(ampl_of), F,
                                                 int(sync) & 0xff, float(ampl), int(lanes), _dptr(status)), "lorahip_mod_frames_sched")
        return status

    def add_awgn(self, iq, sigma, seed=0):
        """complex AWGN (per-component sigma) added in place to a complex64 device tensor"""
        self.use_torch_stream()
        check(self._lib.lorahip_add_awgn(self._h, _dptr(iq), iq.numel(), float(sigma), int(seed) & (2 ** 64 - 1)), "lorahip_add_awgn")
        return iq


def pinned_empty(shape, dtype=np.complex64):
    """numpy array in pinned host memory (lorahip_host_alloc): the host-pointer entry points -- Context.detect_batch_host,
    LoRaDemod.work on host streams -- hand such buffers to the DMA engine directly instead of staging them first"""
    import weakref
    lib = load()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = lib.lorahip_host_alloc(max(n, 1))
    if not ptr:
        raise MemoryError("lorahip_host_alloc(%d)" % n)
    buf = (C.c_char * max(n, 1)).from_address(ptr)
    weakref.finalize(buf, lib.lorahip_host_free, C.c_void_p(ptr))
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


class MixedDetector(_Handle):
    """Channels of different spreading factors demodulated in one call (lorahip_mixed_*: buckets by SF, one stream per bucket,
    concurrent launches, event join -- all below Python). channel_sf: SF of every channel; plan(offsets, S): channel c's S
    back-to-back windows start at sample offsets[c] of the IQ buffer. detect(iq) -> dict of (rows, S) device tensors in
    bucket-major order; rows[c] is channel c's row."""

    _destroy = "lorahip_mixed_destroy"

    def __init__(self, channel_sf, device=0):
        super().__init__()
        sf = np.ascontiguousarray(channel_sf, np.int32).reshape(-1)
        check(self._lib.lorahip_mixed_create(C.byref(self._h), int(device), sf.ctypes.data, sf.size), "lorahip_mixed_create")
        self.n_channels, self.device, self.S = int(sf.size), int(device), 0
        self.rows = np.empty(sf.size, np.int64)
        check(self._lib.lorahip_mixed_rows(self._h, self.rows.ctypes.data), "lorahip_mixed_rows")
        self.buckets = []
        for i in range(self._lib.lorahip_mixed_num_buckets(self._h)):
            s_, r_, n_ = C.c_int32(), C.c_size_t(), C.c_size_t()
            check(self._lib.lorahip_mixed_bucket(self._h, i, C.byref(s_), C.byref(r_), C.byref(n_)), "lorahip_mixed_bucket")
            self.buckets.append((s_.value, r_.value, n_.value))

    def set_variant(self, variant):
        for i in range(len(self.buckets)):
            check(self._lib.lorahip_set_variant(C.c_void_p(self._lib.lorahip_mixed_context(self._h, i)), int(variant)), "lorahip_set_variant")

    def plan(self, channel_offset, windows_per_channel):
        off = np.ascontiguousarray(channel_offset, np.int64).reshape(-1)
        if off.size != self.n_channels:
            raise ValueError("one offset per channel")
        check(self._lib.lorahip_mixed_plan(self._h, off.ctypes.data, int(windows_per_channel)), "lorahip_mixed_plan")
        self.S = int(windows_per_channel)

    def new_outputs(self):
        import torch
        dev = torch.device("cuda", self.device)
        shape = (self.n_channels, self.S)
        return dict(sym=torch.empty(shape, dtype=torch.int16, device=dev), power=torch.empty(shape, dtype=torch.float32, device=dev),
                    powerAvg=torch.empty(shape, dtype=torch.float32, device=dev), fIndex=torch.empty(shape, dtype=torch.float32, device=dev))

    def detect(self, iq, out=None, sync=True):
        """asynchronous unless sync: the buckets run on their own streams; the caller's stream must have finished producing iq"""
        import torch
        out = out or self.new_outputs()
        # the buckets launch on private non-blocking streams: whatever torch's current stream still has queued -- the producer of
        # `iq`, the previous owner of the recycled output blocks -- must be finished first (as LoRaDemod.packets_device does)
        torch.cuda.current_stream(self.device).synchronize()
        check(self._lib.lorahip_mixed_detect(self._h, _dptr(iq), _dptr(out["sym"]), _dptr(out["power"]), _dptr(out["powerAvg"]), _dptr(out["fIndex"])),
              "lorahip_mixed_detect")
        if sync:
            self.synchronize()
        return out

    def synchronize(self):
        check(self._lib.lorahip_mixed_synchronize(self._h), "lorahip_mixed_synchronize")


def shard_plan(channel_sf, n_shards):
    """lorahip_shard_plan (host-only): the shard of every channel under the library's byte-weighted rule -- the C twin of
    lora_sdr_amd.shard.shard_channels, used by lorahip_mixed_create_multi"""
    lib = load()
    sf = np.ascontiguousarray(channel_sf, np.int32).reshape(-1)
    out = np.zeros(sf.size, np.int32)
    check(lib.lorahip_shard_plan(sf.ctypes.data if sf.size else None, sf.size, int(n_shards), out.ctypes.data if sf.size else None), "lorahip_shard_plan")
    return out


class MixedDetectorMulti(_Handle):
    """lorahip_mixed_create_multi: mixed-SF channels over several devices of ONE process (one scheduler, host thread and set of
    streams per device, no data-path collective). devices: list of device indices (may repeat). shard_of[c] = index into devices of
    channel c, rows[c] = its row in that device's result arrays, channels_of(s) = shard s's channels in row order per bucket."""

    _destroy = "lorahip_mixed_destroy"

    def __init__(self, channel_sf, devices):
        super().__init__()
        sf = np.ascontiguousarray(channel_sf, np.int32).reshape(-1)
        dv = np.ascontiguousarray(devices, np.int32).reshape(-1)
        check(self._lib.lorahip_mixed_create_multi(C.byref(self._h), dv.ctypes.data, dv.size, sf.ctypes.data, sf.size), "lorahip_mixed_create_multi")
        self.n_channels, self.devices, self.S = int(sf.size), [int(d) for d in dv], 0
        self.shard_of = np.empty(sf.size, np.int32)
        check(self._lib.lorahip_mixed_shard_of(self._h, self.shard_of.ctypes.data), "lorahip_mixed_shard_of")
        self.rows = np.empty(sf.size, np.int64)
        check(self._lib.lorahip_mixed_rows(self._h, self.rows.ctypes.data), "lorahip_mixed_rows")
        self.counts = []
        for s in range(len(self.devices)):
            d_, n_ = C.c_int32(), C.c_size_t()
            check(self._lib.lorahip_mixed_device(self._h, s, C.byref(d_), C.byref(n_)), "lorahip_mixed_device")
            self.counts.append(int(n_.value))

    def plan(self, channel_offset, windows_per_channel):
        """channel_offset[c]: first sample of channel c inside the IQ buffer of ITS device"""
        off = np.ascontiguousarray(channel_offset, np.int64).reshape(-1)
        if off.size != self.n_channels:
            raise ValueError("one offset per channel")
        check(self._lib.lorahip_mixed_plan(self._h, off.ctypes.data, int(windows_per_channel)), "lorahip_mixed_plan")
        self.S = int(windows_per_channel)

    def new_outputs(self):
        import torch
        outs = []
        for s, dev_i in enumerate(self.devices):
            dev = torch.device("cuda", dev_i)
            shape = (self.counts[s], self.S)
            outs.append(dict(sym=torch.empty(shape, dtype=torch.int16, device=dev), power=torch.empty(shape, dtype=torch.float32, device=dev),
                             powerAvg=torch.empty(shape, dtype=torch.float32, device=dev), fIndex=torch.empty(shape, dtype=torch.float32, device=dev)))
        return outs

    def detect(self, iqs, outs=None, sync=True):
        """iqs: one device tensor per shard (None where a shard has no channel); returns the per-shard output dicts"""
        import torch
        outs = outs or self.new_outputs()
        for dev_i in set(self.devices):
            torch.cuda.synchronize(dev_i)                           # inputs and recycled output blocks are ready (the shards run on private streams)
        n = len(self.devices)

        def arr(ts):
            return (C.c_void_p * n)(*[(t.data_ptr() if t is not None and t.numel() else None) for t in ts])
        check(self._lib.lorahip_mixed_detect_multi(self._h, arr(iqs), arr([o["sym"] for o in outs]), arr([o["power"] for o in outs]),
                                                   arr([o["powerAvg"] for o in outs]), arr([o["fIndex"] for o in outs])), "lorahip_mixed_detect_multi")
        if sync:
            check(self._lib.lorahip_mixed_synchronize(self._h), "lorahip_mixed_synchronize")
        return outs


def design_lowpass(decim, n_taps, cutoff=None):
    """Windowed-sinc (Blackman-Harris) low-pass prototype for the channeliser, unit DC gain; cutoff in cycles per input
    sample (default 0.5/decim = half the channel rate)."""
    fc = 0.5 / decim if cutoff is None else float(cutoff)
    t = np.arange(n_taps) - 0.5 * (n_taps - 1)
    a = 2.0 * np.pi * np.arange(n_taps) / max(n_taps - 1, 1)
    win = 0.35875 - 0.48829 * np.cos(a) + 0.14128 * np.cos(2 * a) - 0.01168 * np.cos(3 * a)
    h = 2.0 * fc * np.sinc(2.0 * fc * t) * (win if n_taps > 1 else 1.0)
    return (h / h.sum()).astype(np.float32)


class Channelizer(_Handle):
    """K channels out of one wideband complex64 stream: mix each centre frequency (cycles per input sample) to 0, low-pass,
    keep every decim-th sample; output (K, n_out) in the layout LoRaDemod.work() takes. Stateful: consecutive run() calls
    continue one stream (filter history and mixer phase carried), reset() starts a new one. See include/lorahip.h."""

    _destroy = "lorahip_channelizer_destroy"

    def __init__(self, ctx, freqs, decim, taps):
        super().__init__()
        self._ctx = ctx                                                  # borrowed: device and stream
        f = np.ascontiguousarray(freqs, np.float64).reshape(-1)
        t = np.ascontiguousarray(taps, np.float32).reshape(-1)
        check(self._lib.lorahip_channelizer_create(C.byref(self._h), ctx._h, f.size, f.ctypes.data, int(decim), t.ctypes.data, t.size),
              "lorahip_channelizer_create")
        self.n_channels, self.decim, self.n_taps = int(f.size), int(decim), int(t.size)

    def reset(self):
        check(self._lib.lorahip_channelizer_reset(self._h), "lorahip_channelizer_reset")

    def out_count(self, n_in):
        return int(self._lib.lorahip_channelizer_out_count(self._h, int(n_in)))

    def run(self, wide, out=None):
        """wide: 1-D complex64 device tensor (the next samples of the stream); returns the (K, n_out) complex64 tensor"""
        return _chan_run(self, "lorahip_channelizer_run", wide, out)

    def run_int(self, wide, scale=None, out=None):
        """run() on integer samples as a radio or a recording hands them out: wide an (n, 2) int16 or int8 device tensor (I, Q; it may
        be buf[k:] of a larger tensor), sample = scale * (float)(I, Q) with scale None = 2^-15 / 2^-7. Converted in the kernel's load:
        bit-identical to run() on the complex64 tensor scale * wide.float(), and free to alternate with run() on one stream."""
        return _chan_run(self, "lorahip_channelizer_run_iq", wide, out, (scale,))

    def run_captures(self, wide):
        """wide: (S, n_in) complex64 device tensor of S independent captures -> (S, K, n_in // decim) tensor, one launch; every
        capture is processed like a fresh stream, the object's own stream state is left alone"""
        import torch
        if wide.dim() != 2 or wide.dtype != torch.complex64:
            raise ValueError("wide must be a (captures, samples) complex64 device tensor")
        wide = wide.contiguous()
        return self._run_captures("lorahip_channelizer_run_captures", wide, (), int(wide.shape[1]))

    def run_captures_int(self, wide, scale=None):
        """run_captures() on integer samples: wide an (S, n_in, 2) int16 or int8 device tensor (captures a whole number of samples
        apart: it may be buf[:, :n_in] of a larger tensor), scale as in run_int; bit-identical to run_captures() on scale * wide.float()"""
        iq = _iq_args(wide, scale, 1)
        return self._run_captures("lorahip_channelizer_run_captures_iq", wide, iq, int(wide.stride(0)) // 2 if wide.shape[0] > 1 and wide.numel() else int(wide.shape[1]))

    def _run_captures(self, run, wide, iq, capture_stride):
        import torch
        S, n_in = int(wide.shape[0]), int(wide.shape[1])
        n_out = n_in // self.decim
        out = torch.empty((S, self.n_channels, n_out), dtype=torch.complex64, device=wide.device)
        self._ctx.use_torch_stream()
        got = C.c_size_t()
        check(getattr(self._lib, run)(self._h, C.c_void_p(wide.data_ptr()) if wide.numel() else None, *iq, S, capture_stride, n_in,
                                      C.c_void_p(out.data_ptr()) if out.numel() else None, n_out, C.byref(got)), run)
        return out


RADIX5_BINS = (5, 10, 20, 40, 80, 160, 320)


def uniform_plan(sample_rate_hz, centre_hz, channel_hz, spacing_hz=200e3, bandwidth_hz=125e3):
    """(n_bins, decim, bins) of a uniform channel plan for PolyphaseChannelizer.for_plan and PolyphaseSynthesizer.for_plan (interp =
    decim): channels bandwidth_hz wide on a grid of spacing_hz round centre_hz, received or generated at sample_rate_hz. n_bins =
    fs / spacing, decim = fs / bandwidth (the demodulator takes its input, and the modulator gives its output, at exactly the
    bandwidth), bins[i] = (channel_hz[i] - centre_hz) / spacing. Host only. ValueError, with the reason, when
    one of the three is no integer (to 1e-9 relative), n_bins is neither a power of two 8..1024 nor 5 * 2^a (a = 0..6), decim is
    outside 1..4096, or a channel lies outside the band (|bin| > n_bins / 2)."""
    fs, spacing, bw = float(sample_rate_hz), float(spacing_hz), float(bandwidth_hz)
    if not (fs > 0 and spacing > 0 and bw > 0):
        raise ValueError("uniform_plan: sample rate, spacing and bandwidth must be positive")

    def whole(value, what):
        value = np.asarray(value, np.float64)
        near = np.rint(value)
        if not np.all(np.isfinite(value)) or np.any(np.abs(value - near) > 1e-9 * np.maximum(1.0, np.abs(value))):
            raise ValueError("uniform_plan: %s is not an integer (%s)" % (what, np.array2string(value, threshold=8)))
        return near.astype(np.int64)

    n_bins = int(whole(fs / spacing, "n_bins = sample rate / spacing"))
    decim = int(whole(fs / bw, "decim = sample rate / bandwidth"))
    ch = np.ascontiguousarray(channel_hz, np.float64).reshape(-1)
    bins = whole((ch - float(centre_hz)) / spacing, "a bin = (channel - centre) / spacing: the centre is off the channel grid, and it")
    if not ((8 <= n_bins <= 1024 and n_bins & (n_bins - 1) == 0) or n_bins in RADIX5_BINS):
        raise ValueError("uniform_plan: n_bins = %d is neither a power of two 8..1024 nor one of %s" % (n_bins, list(RADIX5_BINS)))
    if not 1 <= decim <= 4096:
        raise ValueError("uniform_plan: decim = %d is outside 1..4096" % decim)
    if bins.size and np.abs(bins).max() > n_bins / 2:
        raise ValueError("uniform_plan: a channel is out of band (|bin| = %d > n_bins / 2 = %g)" % (np.abs(bins).max(), n_bins / 2))
    return n_bins, decim, bins.astype(np.int32)


def _plan_bins(n_bins, bins):
    """the int32 bin list of a polyphase bank: `bins`, which must fit 32 bits, or all n_bins bins in order for None"""
    if bins is None:
        return np.arange(int(n_bins) if 0 < int(n_bins) <= 1024 else 0, dtype=np.int32)
    b64 = np.ascontiguousarray(bins, np.int64).reshape(-1)
    if b64.size and (b64.min() < -2 ** 31 or b64.max() >= 2 ** 31):
        raise ValueError("bins must fit 32 bits")
    return b64.astype(np.int32)


def _iq_args(wide, scale, lead):
    """The integer wideband tensor of run_int (lead = 0: (n, 2)) and run_captures_int (lead = 1: (S, n, 2)) checked, and the (format,
    scale) arguments of the *_run_iq entry points: the format from the dtype, scale None = 2^-15 for int16 and 2^-7 for int8. The
    last axis is I, Q; a sample is one element pair, so the tensor may start at any sample of a larger buffer (buf[k:])."""
    import torch
    formats = {torch.int16: (_lib.IQ_SC16, 2.0 ** -15), torch.int8: (_lib.IQ_SC8, 2.0 ** -7)}
    shape = "(captures, samples, 2)" if lead else "(samples, 2)"
    if (not _is_torch(wide) or not wide.is_cuda or wide.dtype not in formats or wide.dim() != lead + 2 or wide.shape[-1] != 2
            or (wide.numel() and (wide.stride(-1) != 1 or wide.stride(-2) != 2))
            or (lead and wide.numel() and wide.shape[0] > 1 and (wide.stride(0) % 2 or wide.stride(0) < 2 * wide.shape[1]))):
        raise ValueError("wide must be a %s int16 or int8 device tensor, the last axis I, Q, with strides (2, 1)%s"
                         % (shape, " and captures a whole number of samples apart" if lead else ""))
    fmt, default = formats[wide.dtype]
    if scale is None:
        scale = default
    try:
        scale = float(scale)
    except (TypeError, ValueError):
        scale = float("nan")
    with np.errstate(over="ignore"):
        held = np.isfinite(np.float32(scale))
    if not held:
        raise ValueError("scale must be a finite real number that float32 holds (None: 2^-15 for int16, 2^-7 for int8)")
    return fmt, C.c_float(scale)


def _chan_run(obj, run, wide, out, int_scale=()):
    """Channelizer.run / run_int and PolyphaseChannelizer.run / run_int: check wide and out, call the C entry point `run`, return the
    outputs it wrote. int_scale = (scale,): wide is the integer tensor of run_int and `run` the *_run_iq entry point."""
    import torch
    if int_scale:
        iq = _iq_args(wide, int_scale[0], 0)
        n_in = int(wide.shape[0])
    else:
        if wide.dim() != 1 or wide.dtype != torch.complex64:
            raise ValueError("wide must be a 1-D complex64 device tensor")
        wide = wide.contiguous()
        iq, n_in = (), wide.numel()
    n_out = obj.out_count(n_in)
    if out is None:
        out = torch.empty((obj.n_channels, n_out), dtype=torch.complex64, device=wide.device)
    elif (out.dim() != 2 or out.shape[0] != obj.n_channels or out.shape[1] < n_out or out.dtype != torch.complex64
          or (out.numel() and (out.stride(1) != 1 or out.stride(0) < out.shape[1]))):
        raise ValueError("out must be a (K, >= n_out) complex64 tensor with unit column stride (rows may be a slice of a wider buffer)")
    obj._ctx.use_torch_stream()
    got = C.c_size_t()
    # the row stride is the tensor's own: `out` may be the columns [w, w + n) of a (K, capacity) buffer that fills chunk by chunk
    check(getattr(obj._lib, run)(obj._h, C.c_void_p(wide.data_ptr()) if wide.numel() else None, *iq, n_in,
                                 C.c_void_p(out.data_ptr()) if out.numel() else None,
                                 int(out.stride(0)) if out.numel() and out.shape[0] > 1 else int(out.shape[1]), C.byref(got)), run)
    return out[:, :got.value]


def _is_cf32_rows(t, n_rows, min_cols=0):
    """t is an (n_rows, >= min_cols) complex64 DEVICE tensor with unit column stride (its rows may be a column slice of a wider
    buffer): what the synthesisers and the resampler take as rows, and the resampler also as out"""
    import torch
    return (_is_torch(t) and t.is_cuda and t.dim() == 2 and t.dtype == torch.complex64 and t.shape[0] == n_rows and t.shape[1] >= min_cols
            and not (t.numel() and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]))))


def _iq_out_args(rows, n_channels, dtype, scale):
    """The arguments of Synthesizer.run_int / PolyphaseSynthesizer.run_int checked before any call into the library, and the (format,
    scale) arguments of the *_run_iq entry points of the transmit side: rows a (K, n) complex64 DEVICE tensor, the format from dtype
    (torch.int16 / torch.int8), scale None = 32767 for int16 and 127 for int8 (|component| <= 1 never clips)."""
    import torch
    formats = {torch.int16: (_lib.IQ_SC16, 32767.0), torch.int8: (_lib.IQ_SC8, 127.0)}
    if dtype not in formats:
        raise ValueError("dtype must be torch.int16 or torch.int8")
    fmt, default = formats[dtype]
    if scale is None:
        scale = default
    try:
        scale = float(scale)
    except (TypeError, ValueError):
        scale = float("nan")
    with np.errstate(over="ignore"):
        held = np.isfinite(np.float32(scale))
    if not held:
        raise ValueError("scale must be a finite real number that float32 holds (None: 32767 for int16, 127 for int8)")
    if not _is_cf32_rows(rows, n_channels):
        raise ValueError("rows must be a (K, n) complex64 device tensor with unit column stride (rows may be a slice of a wider buffer)")
    return fmt, C.c_float(scale)


def _iq_out_buffer(out, dtype, n_out, device):
    """the (>= n_out, 2) integer tensor run_int writes: `out` checked (a device tensor of `dtype`, the last axis I, Q, strides (2, 1);
    it may start at any sample of a larger buffer: buf[k:]), or a new one"""
    import torch
    if out is None:
        return torch.empty((n_out, 2), dtype=dtype, device=device)
    if (not _is_torch(out) or not out.is_cuda or out.dtype != dtype or out.dim() != 2 or out.shape[1] != 2 or out.shape[0] < n_out
            or (out.numel() and (out.stride(1) != 1 or out.stride(0) != 2))):
        raise ValueError("out must be a (>= n * interp, 2) device tensor of dtype %s, the last axis I, Q, with strides (2, 1)" % dtype)
    return out


def _synth_run(obj, run, rows, out, int_format=()):
    """Synthesizer.run / run_int and PolyphaseSynthesizer.run / run_int: check rows and out, call the C entry point `run`, return the
    outputs it wrote. int_format = (dtype, scale): the integer output of run_int and `run` the *_run_iq entry point."""
    import torch
    if int_format:
        iq = _iq_out_args(rows, obj.n_channels, *int_format)
    elif not _is_cf32_rows(rows, obj.n_channels):
        raise ValueError("rows must be a (K, n) complex64 device tensor with unit column stride (rows may be a slice of a wider buffer)")
    n_in = int(rows.shape[1])
    n_out = obj.out_count(n_in)
    if int_format:
        out = _iq_out_buffer(out, int_format[0], n_out, rows.device)
    elif out is None:
        out = torch.empty(n_out, dtype=torch.complex64, device=rows.device)
    elif out.dim() != 1 or out.dtype != torch.complex64 or out.numel() < n_out or (out.numel() and out.stride(0) != 1):
        raise ValueError("out must be a 1-D complex64 tensor of >= n * interp samples with unit stride")
    obj._ctx.use_torch_stream()
    got = C.c_size_t()
    # the row stride is the tensor's own: `rows` may be a column slice of a (K, capacity) buffer
    check(getattr(obj._lib, run)(obj._h, C.c_void_p(rows.data_ptr()) if rows.numel() else None,
                                 int(rows.stride(0)) if rows.numel() and rows.shape[0] > 1 else n_in, n_in,
                                 C.c_void_p(out.data_ptr()) if out.numel() else None, *(iq if int_format else ()), C.byref(got)), run)
    return out[:got.value]


def _synth_clipped(obj, entry):
    """Synthesizer.clipped / PolyphaseSynthesizer.clipped: the count the C entry point reports (it waits for the context's stream)"""
    obj._ctx.use_torch_stream()
    n = C.c_ulonglong()
    check(getattr(obj._lib, entry)(obj._h, C.byref(n)), entry)
    return int(n.value)


class _PolyphaseBank(_Handle):
    """What PolyphaseChannelizer and PolyphaseSynthesizer share. The C entry points are lorahip_<_bank>_*: ..._create takes the powers
    of two, ..._create_radix5 the counts 5 * 2^a; the rate change is the attribute `_rate` names; the synthesiser also passes gains."""

    _bank = None        # "pfb" / "psb"
    _rate = None        # "decim" / "interp"

    def _build(self, radix5, ctx, n_bins, rate, taps, bins, *gains):
        """create the handle and set the attributes"""
        super().__init__()
        self._ctx = ctx                                                  # borrowed: device and stream
        t = np.ascontiguousarray(taps, np.float32).reshape(-1)
        b = _plan_bins(n_bins, bins)
        g = [None if x is None else np.ascontiguousarray(x, np.float32).reshape(-1) for x in gains]
        if any(x is not None and x.size != b.size for x in g):
            raise ValueError("one gain per channel")
        create = "lorahip_%s_create%s" % (self._bank, "_radix5" if radix5 else "")
        check(getattr(self._lib, create)(C.byref(self._h), ctx._h, int(n_bins), None if bins is None else b.ctypes.data,
                                         int(n_bins) if bins is None else b.size, *[None if x is None else x.ctypes.data for x in g],
                                         int(rate), t.ctypes.data, t.size), create)
        self.n_bins, self.n_taps, self.n_channels = int(n_bins), int(t.size), int(b.size)
        setattr(self, self._rate, int(rate))
        self.bins = b
        self.freqs = b.astype(np.float64) / float(self.n_bins)

    @classmethod
    def _radix5(cls, *args):
        self = cls.__new__(cls)
        self._build(True, *args)
        return self

    @classmethod
    def _for_plan(cls, ctx, plan, taps, *gains):
        n_bins, rate, bins = plan
        make = cls.radix5 if int(n_bins) in RADIX5_BINS else cls
        return make(ctx, n_bins, rate, taps, bins, *gains)

    def reset(self):
        check(getattr(self._lib, "lorahip_%s_reset" % self._bank)(self._h), "lorahip_%s_reset" % self._bank)

    def out_count(self, n_in):
        return int(getattr(self._lib, "lorahip_%s_out_count" % self._bank)(self._h, int(n_in)))


class PolyphaseChannelizer(_PolyphaseBank):
    """The channeliser for a uniform channel plan: rows on the grid fs / n_bins (n_bins a power of two, 8..1024; 5 * 2^a, a = 0..6,
    the 200 kHz LoRaWAN grids, through PolyphaseChannelizer.radix5 or .for_plan), row i at centre
    bins[i] / n_bins cycles per input sample (any integers, taken modulo n_bins; negative = the lower half of the band; None: all
    n_bins bins in order). One polyphase fold and one n_bins-point FFT per output time serve every row, so the cost does not grow with
    the number of channels as Channelizer's does. Row i is by definition Channelizer(ctx, [bins[i] / n_bins], decim, taps)'s; .freqs is
    the array a Channelizer or a Synthesizer takes for the same plan. Stateful like Channelizer: consecutive run() calls continue one
    stream, bit-identical to one call; reset() starts a new one. See include/lorahip.h."""

    _bank, _rate, _destroy = "pfb", "decim", "lorahip_pfb_destroy"

    def __init__(self, ctx, n_bins, decim, taps, bins=None):
        self._build(False, ctx, n_bins, decim, taps, bins)

    @classmethod
    def radix5(cls, ctx, n_bins, decim, taps, bins=None):
        """the same object on n_bins = 5 * 2^a bins (5, 10, 20, 40, 80, 160, 320; lorahip_pfb_create_radix5): channels 200 kHz apart
        and 125 kHz wide have decim / n_bins = 8 / 5. The constructor takes the powers of two only, this the seven counts only."""
        return cls._radix5(ctx, n_bins, decim, taps, bins)

    @classmethod
    def for_plan(cls, ctx, plan, taps):
        """the object for plan = (n_bins, decim, bins) as uniform_plan returns it: the constructor or radix5, by n_bins"""
        return cls._for_plan(ctx, plan, taps)

    def run(self, wide, out=None):
        """wide: 1-D complex64 device tensor (the next samples of the stream); returns the (K, n_out) complex64 tensor (written into
        out if given: it may be the columns [w, w + n) of a (K, capacity) buffer)"""
        return _chan_run(self, "lorahip_pfb_run", wide, out)

    def run_int(self, wide, scale=None, out=None):
        """run() on integer samples: wide an (n, 2) int16 or int8 device tensor (I, Q; it may be buf[k:] of a larger tensor), sample =
        scale * (float)(I, Q) with scale None = 2^-15 / 2^-7. Converted in the kernel's load: bit-identical to run() on the complex64
        tensor scale * wide.float(), and free to alternate with run() on one stream. Serves the constructor, radix5 and for_plan."""
        return _chan_run(self, "lorahip_pfb_run_iq", wide, out, (scale,))


class Synthesizer(_Handle):
    """K channel-rate complex64 streams onto their carriers in one wideband stream: zero-stuff by interp, low-pass with taps, mix each
    row up to its centre frequency (cycles per OUTPUT sample: the array a Channelizer of decim = interp takes), scale by gains (None:
    all 1), sum. The mirror image of Channelizer; pass interp * design_lowpass(interp, n_taps, ...) for unit passband gain. Stateful:
    consecutive run() calls continue one stream (filter history and mixer phase carried, bit-identical to one call), reset() starts a
    new one. See include/lorahip.h."""

    _destroy = "lorahip_synthesizer_destroy"

    def __init__(self, ctx, freqs, interp, taps, gains=None):
        super().__init__()
        self._ctx = ctx                                                  # borrowed: device and stream
        f = np.ascontiguousarray(freqs, np.float64).reshape(-1)
        t = np.ascontiguousarray(taps, np.float32).reshape(-1)
        g = None if gains is None else np.ascontiguousarray(gains, np.float32).reshape(-1)
        if g is not None and g.size != f.size:
            raise ValueError("one gain per channel")
        check(self._lib.lorahip_synthesizer_create(C.byref(self._h), ctx._h, f.size, f.ctypes.data, None if g is None else g.ctypes.data,
                                                   int(interp), t.ctypes.data, t.size), "lorahip_synthesizer_create")
        self.n_channels, self.interp, self.n_taps = int(f.size), int(interp), int(t.size)

    def reset(self):
        check(self._lib.lorahip_synthesizer_reset(self._h), "lorahip_synthesizer_reset")

    def out_count(self, n_in):
        return int(self._lib.lorahip_synthesizer_out_count(self._h, int(n_in)))

    def run(self, rows, out=None):
        """rows: (K, n) complex64 device tensor with unit column stride (the next n samples of every channel; may be the columns
        [a, a + n) of a wider buffer); returns the 1-D complex64 tensor of n * interp wideband samples (written into out if given)"""
        return _synth_run(self, "lorahip_synthesizer_run", rows, out)

    def run_int(self, rows, dtype=None, scale=None, out=None):
        """run() with the wideband output as integers, as a DAC, an SDR transmit port or a recording takes them: returns the (n * interp,
        2) device tensor of dtype torch.int16 (the default) or torch.int8, last axis I, Q (written into out if given: a (>= n * interp,
        2) tensor of that dtype with strides (2, 1), which may be buf[k:] of a larger buffer). Each component is scale * c, rounded to
        nearest (ties to even) and saturated, NaN -> 0; scale None = 32767 / 127. Quantised in the kernel's store: bit-identical to
        run()'s output quantised that way (include/lorahip.h), and free to alternate with run() on one stream. clipped() counts."""
        import torch
        return _synth_run(self, "lorahip_synthesizer_run_iq", rows, out, (torch.int16 if dtype is None else dtype, scale))

    def clipped(self):
        """components (I and Q counted separately) that run_int saturated or found NaN since the object was made or reset; waits for
        the stream"""
        return _synth_clipped(self, "lorahip_synthesizer_clipped")


class PolyphaseSynthesizer(_PolyphaseBank):
    """The synthesiser for a uniform channel plan: row k goes to centre bins[k] / n_bins cycles per OUTPUT sample (n_bins a power of
    two, 8..1024; 5 * 2^a, a = 0..6, the 200 kHz LoRaWAN grids, through PolyphaseSynthesizer.radix5 or .for_plan; bins any integers,
    taken modulo n_bins; negative = the lower half of the band; rows that share a bin are summed; None: all n_bins bins in order),
    scaled by gains (None: all 1). One inverse n_bins-point FFT per input time and one fold per output serve every row, so the cost
    does not grow with the number of channels as Synthesizer's does, and interp may be 1..4096. The output is by definition
    Synthesizer(ctx, bins / n_bins, interp, taps, gains)'s (with the exact phase bins (n mod n_bins) / n_bins where n_bins is no power
    of two); .freqs is the array a Synthesizer, a Channelizer or a PolyphaseChannelizer's plan takes. Stateful like Synthesizer:
    consecutive run() calls continue one stream, bit-identical to one call; reset() starts a new one. See include/lorahip.h."""

    _bank, _rate, _destroy = "psb", "interp", "lorahip_psb_destroy"

    def __init__(self, ctx, n_bins, interp, taps, bins=None, gains=None):
        self._build(False, ctx, n_bins, interp, taps, bins, gains)

    @classmethod
    def radix5(cls, ctx, n_bins, interp, taps, bins=None, gains=None):
        """the same object on n_bins = 5 * 2^a bins (5, 10, 20, 40, 80, 160, 320; lorahip_psb_create_radix5): channels 200 kHz apart
        and 125 kHz wide have interp / n_bins = 8 / 5. The constructor takes the powers of two only, this the seven counts only."""
        return cls._radix5(ctx, n_bins, interp, taps, bins, gains)

    @classmethod
    def for_plan(cls, ctx, plan, taps, gains=None):
        """the object for plan = (n_bins, decim, bins) as uniform_plan returns it, interp = decim: the constructor or radix5, by n_bins"""
        return cls._for_plan(ctx, plan, taps, gains)

    def run(self, rows, out=None):
        """rows: (K, n) complex64 device tensor with unit column stride (the next n samples of every channel; may be the columns
        [a, a + n) of a wider buffer); returns the 1-D complex64 tensor of n * interp wideband samples (written into out if given)"""
        return _synth_run(self, "lorahip_psb_run", rows, out)

    def run_int(self, rows, dtype=None, scale=None, out=None):
        """run() with the wideband output as integers: the (n * interp, 2) device tensor of dtype torch.int16 (the default) or
        torch.int8, last axis I, Q; dtype, scale and out as in Synthesizer.run_int. Quantised in the kernel's store: bit-identical to
        run()'s output quantised by the definition in include/lorahip.h. Serves the constructor, radix5 and for_plan."""
        import torch
        return _synth_run(self, "lorahip_psb_run_iq", rows, out, (torch.int16 if dtype is None else dtype, scale))

    def clipped(self):
        """components (I and Q counted separately) that run_int saturated or found NaN since the object was made or reset; waits for
        the stream"""
        return _synth_clipped(self, "lorahip_psb_clipped")


class Resampler(_Handle):
    """K rows of complex64 at one rate -> the same rows at up / down times that rate: zero-stuff by up, low-pass with the real taps,
    keep every down-th sample (include/lorahip.h has the definition). The block between the rate a radio delivers and the rates the
    front ends take: Resampler(ctx, 5, 6, taps) turns 2.4 Msps into the 2 Msps of a Channelizer(decim=16), Resampler(ctx, 25, 24, taps)
    61.44 Msps into the 64 Msps of PolyphaseChannelizer.radix5(320, 512), Resampler(ctx, 25, 256, taps, n_rows=K) rows at 1.28 Msps
    into the 125 kHz LoRaDemod reads; behind a Synthesizer the same objects run the other way. Pass Resampler.design(up, down, n_taps)
    for unit passband gain. Stateful: consecutive run() calls continue one stream (position and filter history carried, bit-identical
    to one call; a call may give 0 outputs), reset() starts a new one."""

    _destroy = "lorahip_resampler_destroy"

    def __init__(self, ctx, up, down, taps, n_rows=1):
        super().__init__()
        self._ctx = ctx                                                  # borrowed: device and stream
        t = np.ascontiguousarray(taps, np.float32).reshape(-1)
        check(self._lib.lorahip_resampler_create(C.byref(self._h), ctx._h, int(n_rows), int(up), int(down), t.ctypes.data, t.size),
              "lorahip_resampler_create")
        self.n_rows, self.up, self.down, self.n_taps = int(n_rows), int(up), int(down), int(t.size)

    @staticmethod
    def design(up, down, n_taps):
        """taps for Resampler(ctx, up, down, taps): up * design_lowpass(max(up, down), n_taps) -- unit passband gain, cutoff at the
        lower of the two Nyquist rates"""
        return (float(up) * design_lowpass(max(int(up), int(down)), n_taps)).astype(np.float32)

    @staticmethod
    def plan(up, down, n_taps, n_rows=1):
        """the tiling Resampler(ctx, up, down, taps of n_taps, n_rows) runs on (lorahip_resampler_plan; no device needed): a dict with
        the fields of struct lorahip_resampler_tiling in include/lorahip.h. Raises LoraHipError where the constructor would."""
        t = _lib.ResamplerTiling()
        check(load().lorahip_resampler_plan(int(up), int(down), int(n_taps), int(n_rows), C.byref(t)), "lorahip_resampler_plan")
        return {name: int(getattr(t, name)) for name, _ in t._fields_}

    def reset(self, position=0):
        """a new stream; position > 0: one whose samples before `position` are zeros and whose first sample is number `position`
        (a capture that stays phase-aligned with an earlier recording)"""
        check(self._lib.lorahip_resampler_reset_at(self._h, int(position)), "lorahip_resampler_reset_at")

    def out_count(self, n_in):
        """outputs per row the next run() of n_in samples per row gives"""
        return int(self._lib.lorahip_resampler_out_count(self._h, int(n_in)))

    def run(self, rows, out=None):
        """rows: (K, n) complex64 device tensor with unit column stride (the next n samples of every row; may be the columns
        [a, a + n) of a wider buffer); for n_rows == 1 a 1-D tensor is taken and a 1-D tensor returned. Returns the (K, n_out)
        complex64 tensor (written into out if given: it may be the columns [w, w + n_out) of a (K, capacity) buffer)."""
        return self._run("lorahip_resampler_run", rows, out, ())

    def run_int(self, rows, scale=None, out=None):
        """run() on integer samples: rows a (K, n, 2) int16 or int8 device tensor (I, Q; rows a whole number of samples apart; (n, 2)
        for n_rows == 1), sample = scale * (float)(I, Q) with scale None = 2^-15 / 2^-7. Converted in the kernel's load: bit-identical
        to run() on the complex64 tensor scale * rows.float(), and free to alternate with run() on one stream."""
        flat = _is_torch(rows) and rows.dim() == 2 and self.n_rows == 1
        if flat:
            rows = rows[None]
        return self._run("lorahip_resampler_run_iq", rows, out, _iq_args(rows, scale, 1), flat)

    def _run(self, run, rows, out, iq, flat=False):
        import torch
        if not iq:
            flat = _is_torch(rows) and rows.dim() == 1 and self.n_rows == 1
            if flat:
                rows = rows[None]
            if not _is_cf32_rows(rows, self.n_rows):
                raise ValueError("rows must be a (n_rows, n) complex64 device tensor with unit column stride (rows may be a slice of a wider buffer)")
        elif rows.shape[0] != self.n_rows:
            raise ValueError("rows must hold n_rows = %d rows" % self.n_rows)
        n_in = int(rows.shape[1])
        in_stride = (int(rows.stride(0)) // (2 if iq else 1)) if rows.numel() and rows.shape[0] > 1 else n_in
        n_out = self.out_count(n_in)
        if out is None:
            out = torch.empty((self.n_rows, n_out), dtype=torch.complex64, device=rows.device)
        else:
            if flat and _is_torch(out) and out.dim() == 1:
                out = out[None]
            if not _is_cf32_rows(out, self.n_rows, n_out):
                raise ValueError("out must be a (K, >= n_out) complex64 device tensor with unit column stride (rows may be a slice of a wider buffer)")
        self._ctx.use_torch_stream()
        got = C.c_size_t()
        check(getattr(self._lib, run)(self._h, C.c_void_p(rows.data_ptr()) if rows.numel() else None, *iq, in_stride, n_in,
                                      C.c_void_p(out.data_ptr()) if out.numel() else None,
                                      int(out.stride(0)) if out.numel() and out.shape[0] > 1 else int(out.shape[1]), C.byref(got)), run)
        res = out[:, :got.value]
        return res[0] if flat else res


class LoRaDetector(_Handle):
    """`LoRaDetector<float>` (LoRaDetector.hpp:8-72): feed N samples, detect() -> arg-max bin."""

    _destroy = "lorahip_detector_destroy"

    def __init__(self, N, device=0):
        super().__init__()
        check(self._lib.lorahip_detector_create(C.byref(self._h), int(device), int(N)), "lorahip_detector_create")
        self.N = int(N)

    def feed(self, i, samp):
        samp = complex(samp)
        check(self._lib.lorahip_detector_feed(self._h, int(i), samp.real, samp.imag), "lorahip_detector_feed")

    def detect(self, fft_output=None):
        """returns (index, power, powerAvg, fIndex); fills fft_output (complex64[N]) if given"""
        idx = C.c_size_t()
        p, pa, fi = C.c_float(), C.c_float(), C.c_float()
        out = None
        if fft_output is not None:
            if fft_output.dtype != np.complex64 or fft_output.size != self.N or not fft_output.flags.c_contiguous:
                raise ValueError("fft_output must be a contiguous complex64[N] array")
            out = fft_output.ctypes.data
        check(self._lib.lorahip_detector_detect(self._h, C.byref(idx), C.byref(p), C.byref(pa), C.byref(fi), out),
              "lorahip_detector_detect")
        return idx.value, p.value, pa.value, fi.value


class LoRaDemod(_Handle):
    """B channels of the `/lora/lora_demod` block (LoRaDemod.cpp), same parameters and defaults."""

    _destroy = "lorahip_demod_destroy"

    STATES = ("FRAMESYNC", "DOWNCHIRP0", "DOWNCHIRP1", "QUARTERCHIRP", "DATASYMBOLS")

    def __init__(self, sf=10, n_channels=1, device=0, channel_sf=None, devices=None):
        """channel_sf (one SF per channel) and devices (a list of device indices) make the mixed-SF / multi-device form
        (lorahip_demod_create_mixed): one handle, global channel numbers; sf / n_channels / device are ignored then"""
        super().__init__()
        self._port_bufs = dict(fft=None, dec=None, raw=None)
        self._mtu = 256                                                 # LoRaDemod.cpp:73
        if channel_sf is None:
            check(self._lib.lorahip_demod_create(C.byref(self._h), int(device), int(sf), int(n_channels)),
                  "lorahip_demod_create")
            self.sf, self.N, self.n_channels = int(sf), 1 << int(sf), int(n_channels)
            self._device = int(device)
            self.channel_sf, self.devices = None, [int(device)]
            return
        csf = np.ascontiguousarray(channel_sf, np.int32).reshape(-1)
        dv = np.ascontiguousarray([0] if devices is None else devices, np.int32).reshape(-1)
        check(self._lib.lorahip_demod_create_mixed(C.byref(self._h), dv.ctypes.data, dv.size, csf.ctypes.data, csf.size), "lorahip_demod_create_mixed")
        self.channel_sf, self.devices, self.n_channels = csf.copy(), [int(x) for x in dv], int(csf.size)
        self.sf = int(csf[0]) if (csf == csf[0]).all() else None
        self.N = None if self.sf is None else 1 << self.sf
        self._device = int(dv[0])
        self.part_of = np.empty(csf.size, np.int32)
        self.local_of = np.empty(csf.size, np.int32)
        check(self._lib.lorahip_demod_part_of(self._h, self.part_of.ctypes.data, self.local_of.ctypes.data), "lorahip_demod_part_of")
        self.parts = []                                                 # (device, sf, n_channels, device_slot)
        for i in range(self._lib.lorahip_demod_num_parts(self._h)):
            d_, s_, n_, k_ = C.c_int32(), C.c_int32(), C.c_size_t(), C.c_int32()
            check(self._lib.lorahip_demod_part(self._h, i, C.byref(d_), C.byref(s_), C.byref(n_), C.byref(k_)), "lorahip_demod_part")
            self.parts.append((d_.value, s_.value, n_.value, k_.value))

    @staticmethod
    def make(sf):
        return LoRaDemod(sf)

    def device_slot_of(self):
        """mixed form: for every channel the index into `devices` of the GPU that holds it"""
        return np.array([self.parts[p][3] for p in self.part_of], np.int32)

    def setSync(self, sync):
        check(self._lib.lorahip_demod_set_sync(self._h, int(sync) & 0xff), "lorahip_demod_set_sync")

    def setThreshold(self, thresh_dB):
        check(self._lib.lorahip_demod_set_threshold(self._h, float(thresh_dB)), "lorahip_demod_set_threshold")

    def setMTU(self, mtu):
        check(self._lib.lorahip_demod_set_mtu(self._h, int(mtu)), "lorahip_demod_set_mtu")
        self._mtu = int(mtu)

    def activate(self):
        check(self._lib.lorahip_demod_activate(self._h), "lorahip_demod_activate")

    def set_mode(self, mode):
        """0 auto, 1 streaming kernel (frame machine on the device), 2 host-driven lock-step rounds"""
        check(self._lib.lorahip_demod_set_mode(self._h, int(mode)), "lorahip_demod_set_mode")

    def set_variant(self, variant):
        """kernel variant of the host-driven mode's batch launches; the contracted build (40) is refused at this level"""
        check(self._lib.lorahip_demod_set_variant(self._h, int(variant)), "lorahip_demod_set_variant")

    def set_stream_grid(self, max_workgroups):
        """the streaming kernels' grid (scheduling only, same results): 0 the library's choice, < 0 one workgroup per channel set
        always, n > 0 at most n workgroups each walking several channels (SF11 / SF12)"""
        check(self._lib.lorahip_demod_set_stream_grid(self._h, int(max_workgroups)), "lorahip_demod_set_stream_grid")

    def set_stream_lanes(self, log2_lanes):
        """lanes per channel of the streaming kernels at SF7-9 (scheduling only, same results): 0 by channel count (default), < 0
        always 16 points per lane, 4 / 5 / 6 = 16 / 32 / 64 lanes per channel where the build holds that instance; 16 | l = two groups
        of 2^l lanes per channel, the second one a window ahead of the call (lorahip.h)"""
        check(self._lib.lorahip_demod_set_stream_lanes(self._h, int(log2_lanes)), "lorahip_demod_set_stream_lanes")

    def part_stream_lanes(self):
        """mixed form: log2 of the lanes per channel each part's streaming launches run on, in the order of `parts` (a part counts the
        wavefronts its sibling parts put on the same device: lorahip.h, lorahip_demod_create_mixed)"""
        out = []
        for i in range(len(self.parts)):
            h = self._lib.lorahip_demod_part_handle(self._h, i)
            v = int(self._lib.lorahip_demod_stream_lanes(C.c_void_p(h)))
            if v < 0:
                raise _lib.LoraHipError(v, "lorahip_demod_stream_lanes")
            out.append(v)
        return out

    def stream_lanes(self):
        """log2 of the lanes per channel the streaming launches of this object run on"""
        v = int(self._lib.lorahip_demod_stream_lanes(self._h))
        if v < 0:
            raise _lib.LoraHipError(v, "lorahip_demod_stream_lanes")
        return v

    def set_record_capacity(self, max_calls_per_launch):
        """bound the streaming kernels' per-launch record capacity (0: the library's own sizing): a channel that fills it is resumed by
        another launch, results unchanged -- the tests of the resume path"""
        check(self._lib.lorahip_demod_set_record_capacity(self._h, int(max_calls_per_launch)), "lorahip_demod_set_record_capacity")

    def set_trace(self, on=True):
        check(self._lib.lorahip_demod_set_trace(self._h, int(bool(on))), "lorahip_demod_set_trace")

    def work_segments(self, buf, first_sample, n_samples):
        """lorahip_demod_run_device_segments: channel c's stream is buf.view(-1)[first_sample[c] : first_sample[c] + n_samples[c]] of ONE
        torch complex64 device tensor -- the running receiver behind a channeliser, which advances first_sample[c] by consumed(c)
        and re-presents the remainder with the new samples, without copying anything. Returns the number of lock-step rounds."""
        import torch
        if not _is_torch(buf) or buf.dtype != torch.complex64 or not buf.is_contiguous():
            raise ValueError("expected a contiguous complex64 device tensor")
        first = np.ascontiguousarray(first_sample, np.int64)
        cnt = np.ascontiguousarray(n_samples, np.uint64)
        if first.shape != (self.n_channels,) or cnt.shape != (self.n_channels,):
            raise ValueError("first_sample and n_samples need one entry per channel")
        if cnt.size and int((first + cnt.astype(np.int64)).max()) > buf.numel():
            raise ValueError("a segment ends beyond the buffer")
        rounds = C.c_int64()
        if self.channel_sf is not None:
            # an object of several (device, SF) parts: each part launches on its OWN stream so that they overlap on the device; one
            # common stream would run them one after the other. What torch's stream still has queued -- the producer of `buf` -- ends first.
            torch.cuda.current_stream(buf.device).synchronize()
            check(self._lib.lorahip_demod_run_device_segments(self._h, _dptr(buf), first.ctypes.data_as(C.POINTER(C.c_int64)),
                                                              cnt.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(rounds)), "lorahip_demod_run_device_segments")
            return rounds.value
        check(self._lib.lorahip_demod_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(buf.device).cuda_stream)), "lorahip_demod_set_stream")
        try:
            check(self._lib.lorahip_demod_run_device_segments(self._h, _dptr(buf), first.ctypes.data_as(C.POINTER(C.c_int64)),
                                                              cnt.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(rounds)), "lorahip_demod_run_device_segments")
        finally:
            self._lib.lorahip_demod_reset_stream(self._h)
        return rounds.value

    def work_host_rows(self, rows, first_sample, n_samples):
        """lorahip_demod_run_host_rows: `rows` is a (n_channels, row_stride) complex64 HOST array (pinned_empty() for a straight DMA);
        channel c's stream is rows[c, first_sample[c] : first_sample[c] + n_samples[c]]. One strided copy, then the run."""
        if not isinstance(rows, np.ndarray) or rows.dtype != np.complex64 or rows.ndim != 2 or rows.shape[0] != self.n_channels or not rows.flags.c_contiguous:
            raise ValueError("expected a C-contiguous (n_channels, row_stride) complex64 host array")
        first = np.ascontiguousarray(first_sample, np.int64)
        cnt = np.ascontiguousarray(n_samples, np.uint64)
        if first.shape != (self.n_channels,) or cnt.shape != (self.n_channels,):
            raise ValueError("first_sample and n_samples need one entry per channel")
        rounds = C.c_int64()
        check(self._lib.lorahip_demod_run_host_rows(self._h, rows.ctypes.data, int(rows.shape[1]), first.ctypes.data, cnt.ctypes.data, C.byref(rounds)),
              "lorahip_demod_run_host_rows")
        return rounds.value

    def work_segments_multi(self, bufs, first_sample, n_samples):
        """lorahip_demod_run_device_segments_multi: bufs[s] is the complex64 device tensor on devices[s] that holds the segments of the
        channels of device slot s (None for a slot without channels)"""
        first = np.ascontiguousarray(first_sample, np.int64)
        cnt = np.ascontiguousarray(n_samples, np.uint64)
        if first.shape != (self.n_channels,) or cnt.shape != (self.n_channels,):
            raise ValueError("first_sample and n_samples need one entry per channel")
        import torch
        for b in bufs:
            if b is not None:
                torch.cuda.synchronize(b.device)                    # the parts launch on private streams
        ptrs = (C.c_void_p * len(bufs))(*[(b.data_ptr() if b is not None and b.numel() else None) for b in bufs])
        rounds = C.c_int64()
        check(self._lib.lorahip_demod_run_device_segments_multi(self._h, ptrs, len(bufs), first.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                cnt.ctypes.data_as(C.POINTER(C.c_size_t)), C.byref(rounds)),
              "lorahip_demod_run_device_segments_multi")
        return rounds.value

    def set_signals(self, on=True):
        """keep the block's error / power / snr signals (LoRaDemod.cpp:267-269) without a per-call trace"""
        check(self._lib.lorahip_demod_set_signals(self._h, int(bool(on))), "lorahip_demod_set_signals")

    def signals(self, pos=False):
        """the queued signal emissions as arrays: channel, round, error, power, snr (cleared with the packets); pos=True adds the int64
        sample position at which the emitting call began -- the sync_pos of the frame's packet (lorahip_rx_info), the key match_signals joins on"""
        n = int(self._lib.lorahip_demod_num_signals(self._h))
        ch, rd, er = np.empty(n, np.int32), np.empty(n, np.int64), np.empty(n, np.int32)
        pw, sn = np.empty(n, np.float32), np.empty(n, np.float32)
        check(self._lib.lorahip_demod_get_signals(self._h, ch.ctypes.data, rd.ctypes.data, er.ctypes.data, pw.ctypes.data, sn.ctypes.data, n),
              "lorahip_demod_get_signals")
        if pos:
            ps = np.empty(n, np.int64)
            if n:
                check(self._lib.lorahip_demod_get_signals_pos(self._h, ps.ctypes.data, n), "lorahip_demod_get_signals_pos")
            return ch, rd, er, pw, sn, ps
        return ch, rd, er, pw, sn

    def rewind(self):
        check(self._lib.lorahip_demod_rewind(self._h), "lorahip_demod_rewind")

    def work_append(self, buf, n_valid):
        """lorahip_demod_run_device_append: buf is a (n_channels, capacity) complex64 device tensor of which the first n_valid columns are
        valid; every channel continues at its own read position"""
        import torch
        if not _is_torch(buf) or buf.dim() != 2 or buf.shape[0] != self.n_channels or buf.dtype != torch.complex64 or not buf.is_contiguous():
            raise ValueError("expected a contiguous (n_channels, capacity) complex64 device tensor")
        rounds = C.c_int64()
        check(self._lib.lorahip_demod_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(buf.device).cuda_stream)), "lorahip_demod_set_stream")
        try:
            check(self._lib.lorahip_demod_run_device_append(self._h, _dptr(buf), int(buf.shape[1]), int(n_valid), C.byref(rounds)), "lorahip_demod_run_device_append")
        finally:
            self._lib.lorahip_demod_reset_stream(self._h)
        return rounds.value

    def receiver_rows(self, cap_packets, stride=None, info=False):
        """device tensors for receive(): (cap_packets, stride) int16 symbols, (cap_packets,) int32 lengths and channels; info=True adds a
        fourth, (cap_packets, 4) int64: end_pos, data_pos, sync_pos, freq_error per packet (lorahip_rx_info; RxInfo names the columns),
        which receive() / receive_flush() pass on (not with async_=3: refused)"""
        import torch
        dev = torch.device("cuda", int(self._device))
        if stride is None:
            stride = max(8, min(self._mtu, int(self._lib.lorahip_decode_max_symbols())))      # no packet is longer than the MTU (LoRaDemod.cpp:291)
        rows = (torch.empty((int(cap_packets), int(stride)), dtype=torch.int16, device=dev), torch.empty(int(cap_packets), dtype=torch.int32, device=dev),
                torch.empty(int(cap_packets), dtype=torch.int32, device=dev))
        return rows + (torch.empty((int(cap_packets), 4), dtype=torch.int64, device=dev),) if info else rows

    def receiver_signal_rows(self, cap, pinned_host=False, pos=False):
        """lorahip_demod_receive_signal_rows: with set_signals(True), every receive() / receive_flush() delivers the block's signals
        (error / power / snr once per packet at DOWNCHIRP1, LoRaDemod.cpp:267-269) of the step whose packets it delivers into these
        rows, last_signals() of them. Returns the tensors (channel int32, error int32, power float32, snr float32): device memory, or --
        pinned_host -- numpy arrays over pinned host memory the device writes directly (read them after the stream has passed).
        cap = 0 unregisters (receiver steps drop the signals again). pos=True adds a fifth member, int64: the sample position at which
        the emitting call began (absolute in the channel's row; equals the sync_pos of the frame's packet)."""
        import torch
        r = _lib.SignalRowsPos() if pos else _lib.SignalRows()
        r.struct_size = C.sizeof(r)
        cap = int(cap)
        if cap == 0:
            self._sig_rows = None
            check(self._lib.lorahip_demod_receive_signal_rows(self._h, None), "lorahip_demod_receive_signal_rows")
            return None
        if pinned_host:
            rows = (pinned_empty((cap,), np.int32), pinned_empty((cap,), np.int32), pinned_empty((cap,), np.float32), pinned_empty((cap,), np.float32))
            if pos:
                rows += (pinned_empty((cap,), np.int64),)
                r.pos = rows[4].ctypes.data
            r.channel, r.error, r.power, r.snr = (a.ctypes.data for a in rows[:4])
        else:
            dev = torch.device("cuda", int(self._device))
            rows = (torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                    torch.empty(cap, dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.float32, device=dev))
            if pos:
                rows += (torch.empty(cap, dtype=torch.int64, device=dev),)
                r.pos = rows[4].data_ptr()
            r.channel, r.error, r.power, r.snr = (a.data_ptr() for a in rows[:4])
        r.cap = cap
        check(self._lib.lorahip_demod_receive_signal_rows(self._h, C.byref(r)), "lorahip_demod_receive_signal_rows")
        self._sig_rows = rows                                # (kept alive while registered)
        return rows

    def register_signal_rows(self, rows):
        """register a set made by receiver_signal_rows() again: a caller that alternates two sets of packet rows (pipelined consumers, the
        resident receiver) alternates two sets of signal rows the same way, one registration before each receive()"""
        r = _lib.SignalRowsPos() if len(rows) > 4 else _lib.SignalRows()       # (a fifth member: the positions)
        r.struct_size = C.sizeof(r)
        ptr = (lambda a: a.ctypes.data) if isinstance(rows[0], np.ndarray) else (lambda a: a.data_ptr())
        r.channel, r.error, r.power, r.snr = (ptr(a) for a in rows[:4])
        if len(rows) > 4:
            r.pos = ptr(rows[4])
        r.cap = int(rows[0].shape[0])
        check(self._lib.lorahip_demod_receive_signal_rows(self._h, C.byref(r)), "lorahip_demod_receive_signal_rows")
        self._sig_rows = rows

    def last_steps(self):
        """the resident steps the last receive() / receive_flush() reported, oldest first: [(packets, signals)] (a flush at depth > 1
        reports several, each in the rows of its own call)"""
        pk, sg = (C.c_size_t * 4)(), (C.c_size_t * 4)()
        n = int(self._lib.lorahip_demod_receive_steps(self._h, pk, sg, 4))
        return [(int(pk[i]), int(sg[i])) for i in range(n)]

    def resident_active(self):
        """True while the resident kernel of receive(async_=3) is on the device"""
        return bool(self._lib.lorahip_demod_resident_active(self._h))

    def last_signals(self):
        """signals the last receive() / receive_flush() delivered into the registered signal rows"""
        return int(self._lib.lorahip_demod_receive_num_signals(self._h))

    def _rows_struct(self, rows, async_, depth=0):
        syms, nsyms, chan = rows[:3]
        r = _lib.PacketRowsInfo() if len(rows) > 3 else _lib.PacketRows()      # (a fourth tensor: receiver_rows(info=True))
        r.struct_size = C.sizeof(r)
        if len(rows) > 3:
            r.info_dev = rows[3].data_ptr()
        r.syms_dev, r.sym_stride, r.nsyms_dev, r.channel_dev = syms.data_ptr(), int(syms.shape[1]), nsyms.data_ptr(), chan.data_ptr()
        r.cap_packets, r.async_, r.reserved = int(syms.shape[0]), int(async_), int(depth)
        return r

    def receive(self, buf, n_valid, rows, async_=True, order_with_torch=True, depth=1):
        """lorahip_demod_receive: one receiver step in one call into the library -- the append run, the completed packets packed into
        `rows` (receiver_rows()) on the device, the queue cleared. Returns (n_packets, work_calls). async_: False = wait; True = the
        rows are valid in the order of the stream the object launches on; 2 = PIPELINED: the step is launched and the packets of
        the previous step are returned (receive_flush() delivers the last step's). A pipelined receiver keeps its private stream
        (the steps must stay in flight across calls), ordered against torch's current stream on the device, without a host wait:
        the launch stream follows what torch's stream holds at entry (whatever produced `buf`, whatever still reads the rows of the
        call before: lorahip_demod_stream_follow), and torch's stream waits for the packing of the rows at exit
        (lorahip_demod_stream_wait) -- work queued on it after this call sees the rows. order_with_torch=False leaves both out (two
        event records and two stream waits per step): for a caller that orders its own streams, or times the C entry itself."""
        import torch
        r = self._rows_struct(rows, async_ if async_ in (2, 3) else int(bool(async_)), depth if async_ == 3 else 0)
        n, calls = C.c_size_t(), C.c_int64()
        if async_ == 3:
            # RESIDENT: one kernel stays on the device and takes the steps as messages. The rows passed here are filled by THIS step and
            # are complete when the receive() `depth` calls later (default: the NEXT one) or receive_flush() returns (whose counts are this
            # step's): cycle depth + 1 sets of rows. The kernel reads `buf` on its
            # own: what produced the new samples must have finished (order_with_torch: torch's current stream is waited for).
            if order_with_torch:
                torch.cuda.current_stream(buf.device).synchronize()
            try:
                check(self._lib.lorahip_demod_receive(self._h, _dptr(buf), int(buf.shape[1]), int(n_valid), C.byref(r), C.byref(n), C.byref(calls)), "lorahip_demod_receive")
            except Exception as e:
                e.n_packets = n.value
                raise
            return n.value, calls.value
        if async_ == 2:
            if not order_with_torch:
                check(self._lib.lorahip_demod_receive(self._h, _dptr(buf), int(buf.shape[1]), int(n_valid), C.byref(r), C.byref(n), C.byref(calls)), "lorahip_demod_receive")
                return n.value, calls.value
            ts = C.c_void_p(torch.cuda.current_stream(buf.device).cuda_stream)
            check(self._lib.lorahip_demod_stream_follow(self._h, ts), "lorahip_demod_stream_follow")
            try:
                check(self._lib.lorahip_demod_receive(self._h, _dptr(buf), int(buf.shape[1]), int(n_valid), C.byref(r), C.byref(n), C.byref(calls)), "lorahip_demod_receive")
            except Exception as e:
                e.n_packets = n.value                       # LORAHIP_E_INVALID with rows that are too small: the rows needed (nothing is lost)
                raise
            finally:
                self._lib.lorahip_demod_stream_wait(self._h, ts)
            return n.value, calls.value
        check(self._lib.lorahip_demod_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(buf.device).cuda_stream)), "lorahip_demod_set_stream")
        try:
            check(self._lib.lorahip_demod_receive(self._h, _dptr(buf), int(buf.shape[1]), int(n_valid), C.byref(r), C.byref(n), C.byref(calls)), "lorahip_demod_receive")
        finally:
            self._lib.lorahip_demod_reset_stream(self._h)
        return n.value, calls.value

    def receive_flush(self, rows=None):
        """lorahip_demod_receive_flush: the last pipelined step's packets into `rows` (None: dropped); returns (n_packets, work_calls)
        with the launch stream drained"""
        n, calls = C.c_size_t(), C.c_int64()
        r = self._rows_struct(rows, 0) if rows is not None else None
        if rows is not None:
            import torch
            # (whatever on torch's stream still reads the rows of the call before is ordered before this call's packing)
            check(self._lib.lorahip_demod_stream_follow(self._h, C.c_void_p(torch.cuda.current_stream(rows[0].device).cuda_stream)), "lorahip_demod_stream_follow")
        try:
            check(self._lib.lorahip_demod_receive_flush(self._h, C.byref(r) if r is not None else None, C.byref(n), C.byref(calls)), "lorahip_demod_receive_flush")
        except Exception as e:
            e.n_packets = n.value
            raise
        return n.value, calls.value

    def work(self, streams):
        """Feed one complete input stream per channel and run work() until < 2N samples remain
        everywhere. streams: list of complex64 numpy arrays (one per channel, any lengths), ONE numpy array of shape
        (n_channels, samples) in host memory, or ONE torch complex64 device tensor of that shape. Returns the number of lock-step rounds."""
        rounds = C.c_int64()
        if _is_torch(streams):
            if streams.dim() != 2 or streams.shape[0] != self.n_channels:
                raise ValueError("expected a (n_channels, samples) tensor")
            import torch
            # run on torch's current stream: whatever produced `streams` there is ordered before the demodulator's kernels
            check(self._lib.lorahip_demod_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(streams.device).cuda_stream)),
                  "lorahip_demod_set_stream")
            try:
                check(self._lib.lorahip_demod_run_device(self._h, _dptr(streams), int(streams.shape[1]),
                                                         C.byref(rounds)), "lorahip_demod_run_device")
            finally:
                # torch may destroy that stream later: later calls (numpy work(), packets_device()) use the private one again
                self._lib.lorahip_demod_reset_stream(self._h)
            return rounds.value
        if isinstance(streams, np.ndarray) and streams.ndim == 2:
            # one (n_channels, samples) host array: the per-channel pointers without a Python loop
            if streams.shape[0] != self.n_channels:
                raise ValueError("expected a (n_channels, samples) array")
            a = np.ascontiguousarray(streams, np.complex64)
            ptrs = (np.uint64(a.ctypes.data) + np.arange(self.n_channels, dtype=np.uint64) * np.uint64(a.strides[0]))
            lens = np.full(self.n_channels, a.shape[1], dtype=np.uint64)
            check(self._lib.lorahip_demod_run(self._h, ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), lens.ctypes.data_as(C.POINTER(C.c_size_t)),
                                              C.byref(rounds)), "lorahip_demod_run")
            return rounds.value
        if len(streams) != self.n_channels:
            raise ValueError("expected %d streams" % self.n_channels)
        keep = [np.ascontiguousarray(s, np.complex64).reshape(-1) for s in streams]
        ptrs = (C.c_void_p * self.n_channels)(*[k.ctypes.data for k in keep])
        lens = (C.c_size_t * self.n_channels)(*[k.size for k in keep])
        check(self._lib.lorahip_demod_run(self._h, ptrs, lens, C.byref(rounds)), "lorahip_demod_run")
        return rounds.value

    def packets_arrays(self, clear=True, info=False):
        """The queued packets as four flat arrays -- channel (int32), round (int64), length (int64), and all symbols back to
        back (int16) -- in posting order: what lorahip_demod_get_packets delivers, without per-packet Python objects. info=True adds a
        fifth, (P, 4) int64: end_pos, data_pos, sync_pos, freq_error per packet (lorahip_rx_info; RxInfo names the columns)"""
        n = self._lib.lorahip_demod_num_packets(self._h)
        ns = self._lib.lorahip_demod_num_packet_symbols(self._h)
        ch, rd, ln = np.empty(n, np.int32), np.empty(n, np.int64), np.empty(n, np.int64)
        syms = np.empty(ns, np.int16)
        check(self._lib.lorahip_demod_get_packets(self._h, ch.ctypes.data, rd.ctypes.data, ln.ctypes.data, n, syms.ctypes.data, ns),
              "lorahip_demod_get_packets")
        inf = np.empty((n, 4), np.int64)
        if info and n:
            check(self._lib.lorahip_demod_get_packets_info(self._h, inf.ctypes.data, n), "lorahip_demod_get_packets_info")
        if clear:
            self._lib.lorahip_demod_clear_packets(self._h)
        return (ch, rd, ln, syms, inf) if info else (ch, rd, ln, syms)

    def clear_packets(self):
        """drop the queued packets (what packets*(clear=True) do after reading them)"""
        self._lib.lorahip_demod_clear_packets(self._h)

    def packets(self, clear=True):
        """[(channel, round, int16 symbols)] -- the Pothos::Packet payloads of output port 0"""
        ch, rd, ln, syms = self.packets_arrays(clear)
        parts = np.split(syms, np.cumsum(ln)[:-1]) if ch.size else []       # views into one array: no per-packet copy
        return list(zip(ch.tolist(), rd.tolist(), parts))

    def packets_device(self, stride=None, clear=True, info=False):
        """The queued packets as device tensors in the decoder's input layout -- (P, stride) int16 symbols (zero padded), (P,) int32
        lengths, (P,) int32 channels -- ready for LoRaDecoder.decode_batch(); no per-packet Python work. Straight after a
        work() of the streaming mode the packets never visit the host (rows ordered by channel, then time); otherwise the
        rows follow packets()'s order. stride defaults to the MTU. On a mixed object whose parts share one device: the parts' rows
        one after the other in packets()'s order, each part's as above, with global channel numbers -- the input of
        LoRaDecoderSet.decode_batch(syms, nsyms, index=channels, table=decoder of channel); over several devices: refused.
        info=True adds a fourth tensor, (P, 4) int64: end_pos, data_pos, sync_pos, freq_error per row (lorahip_rx_info)."""
        import torch
        n = int(self._lib.lorahip_demod_num_packets(self._h))
        dev = torch.device("cuda", int(self._device))
        if stride is None:
            stride = max(8, min(self._mtu, int(self._lib.lorahip_decode_max_symbols())))      # no packet is longer than the MTU (LoRaDemod.cpp:291)
        syms = torch.empty((n, int(stride)), dtype=torch.int16, device=dev)      # every element is written (rows are zero padded)
        nsyms = torch.empty(n, dtype=torch.int32, device=dev)
        chan = torch.empty(n, dtype=torch.int32, device=dev)
        inf = torch.empty((n, 4), dtype=torch.int64, device=dev) if info else None
        got = C.c_size_t()
        if n:
            torch.cuda.current_stream(dev).synchronize()            # the blocks may have pending work of their previous owner
            if info:
                check(self._lib.lorahip_demod_packets_to_device_info(self._h, C.c_void_p(syms.data_ptr()), int(stride), C.c_void_p(nsyms.data_ptr()),
                                                                     C.c_void_p(chan.data_ptr()), C.c_void_p(inf.data_ptr()), n, C.byref(got)),
                      "lorahip_demod_packets_to_device_info")
            else:
                check(self._lib.lorahip_demod_packets_to_device(self._h, C.c_void_p(syms.data_ptr()), int(stride), C.c_void_p(nsyms.data_ptr()),
                                                                C.c_void_p(chan.data_ptr()), n, C.byref(got)), "lorahip_demod_packets_to_device")
        if clear:
            self._lib.lorahip_demod_clear_packets(self._h)
        return (syms, nsyms, chan, inf) if info else (syms, nsyms, chan)

    def consumed(self, channel):
        """samples of the channel's stream consumed by the last work()"""
        return int(self._lib.lorahip_demod_consumed(self._h, int(channel)))

    def consumed_all(self):
        """consumed(c) of every channel: an int64 numpy array (one call into the library)"""
        out = np.empty(self.n_channels, np.int64)
        check(self._lib.lorahip_demod_consumed_all(self._h, out.ctypes.data_as(C.POINTER(C.c_int64))), "lorahip_demod_consumed_all")
        return out

    def work_calls(self):
        return int(self._lib.lorahip_demod_work_calls(self._h))

    def kernel_ms(self):
        """device time of the streaming kernel launches of the last work() (HIP events on the launch stream)"""
        return float(self._lib.lorahip_demod_kernel_ms(self._h))

    def last_launches(self):
        """streaming kernel launches the last work() took (1 unless its record buffers filled and the run was resumed)"""
        return int(self._lib.lorahip_demod_last_launches(self._h))

    def near_threshold(self):
        """(near_squelch, near_step): decisions since activate() that sat within float rounding of their boundary -- |snr - thresh|
        <= 4e-5 dB where the squelch is consumed, fine-tune steps within 6e-5 of an integer (include/lorahip.h). Counted, not changed."""
        a, b = C.c_int64(), C.c_int64()
        check(self._lib.lorahip_demod_near_threshold(self._h, C.byref(a), C.byref(b)), "lorahip_demod_near_threshold")
        return a.value, b.value

    def set_fine_gather(self, on):
        """A/B switch: read the fine-tune table in HBM instead of evaluating it from the split tables (include/lorahip.h)"""
        check(self._lib.lorahip_demod_set_fine_gather(self._h, int(bool(on))), "lorahip_demod_set_fine_gather")

    def labels(self, channel):
        """The stream labels the block posts at index 0 of what each work() call produces on raw / dec / fft, one per call
        ("" = none): "SYNC", "P <fIndex>", "DC", "QC", "S<n> <fIndex>" (LoRaDemod.cpp:213,221-224,245,282,302-305,314-319),
        formatted by the library from the per-call trace (set_trace(True) before work())."""
        n, nb = C.c_size_t(), C.c_size_t()
        check(self._lib.lorahip_demod_get_labels(self._h, int(channel), None, 0, C.byref(n), C.byref(nb)), "lorahip_demod_get_labels")
        buf = C.create_string_buffer(max(nb.value, 1))
        check(self._lib.lorahip_demod_get_labels(self._h, int(channel), buf, nb.value, C.byref(n), C.byref(nb)), "lorahip_demod_get_labels")
        out = buf.raw[:nb.value].split(b"\0")[:n.value]
        return [x.decode() for x in out]

    def set_ports(self, fft_frames=0, dec_samples=0, raw_samples=0):
        """Attach the block's debug ports for the next work() calls (LoRaDemod.cpp:81-83): per channel, `fft_frames` frames of N
        FFT bins (one per work() call), `dec_samples` dechirped samples, `raw_samples` consumed samples; 0 = that port off,
        all 0 = ports off. The buffers are device tensors owned by this object; read them with ports(channel)."""
        import torch
        if self.N is None:
            raise ValueError("the debug ports need one spreading factor for all channels (include/lorahip.h)")
        dev = torch.device("cuda", int(self._device))
        B = self.n_channels
        self._port_bufs = dict(
            fft=torch.zeros((B, int(fft_frames), self.N), dtype=torch.complex64, device=dev) if fft_frames else None,
            dec=torch.zeros((B, int(dec_samples)), dtype=torch.complex64, device=dev) if dec_samples else None,
            raw=torch.zeros((B, int(raw_samples)), dtype=torch.complex64, device=dev) if raw_samples else None)
        torch.cuda.synchronize(dev)
        if not (fft_frames or dec_samples or raw_samples):
            check(self._lib.lorahip_demod_set_ports(self._h, None), "lorahip_demod_set_ports")
            return
        p = _lib.DemodPorts()
        p.struct_size = C.sizeof(_lib.DemodPorts)
        b = self._port_bufs
        p.fft_dev, p.fft_cap_frames = (b["fft"].data_ptr() if fft_frames else None), int(fft_frames)
        p.dec_dev, p.dec_cap_samples = (b["dec"].data_ptr() if dec_samples else None), int(dec_samples)
        p.raw_dev, p.raw_cap_samples = (b["raw"].data_ptr() if raw_samples else None), int(raw_samples)
        check(self._lib.lorahip_demod_set_ports(self._h, C.byref(p)), "lorahip_demod_set_ports")

    def ports(self, channel):
        """what the last work() produced on the debug ports of `channel`: dict of device tensors fft (frames, N), dec (samples,),
        raw (samples,) -- cut to what was produced (or to the capacity given to set_ports)"""
        nf, nd, nr = C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(self._lib.lorahip_demod_port_counts(self._h, int(channel), C.byref(nf), C.byref(nd), C.byref(nr)), "lorahip_demod_port_counts")
        b = self._port_bufs
        return dict(fft=None if b["fft"] is None else b["fft"][channel, :min(nf.value, b["fft"].shape[1])],
                    dec=None if b["dec"] is None else b["dec"][channel, :min(nd.value, b["dec"].shape[1])],
                    raw=None if b["raw"] is None else b["raw"][channel, :min(nr.value, b["raw"].shape[1])],
                    produced=dict(fft=nf.value, dec=nd.value, raw=nr.value))

    def trace_array(self, channel):
        """the per-call trace of `channel` as one numpy structured array (fields of lorahip_work_result): no per-call Python objects"""
        n = self._lib.lorahip_demod_trace_len(self._h, int(channel))
        arr = np.zeros(n, dtype=WORK_RESULT_DTYPE)
        if n:
            check(self._lib.lorahip_demod_get_trace(self._h, int(channel), C.cast(arr.ctypes.data, C.POINTER(WorkResult)), n), "lorahip_demod_get_trace")
        return arr

    def trace(self, channel):
        n = self._lib.lorahip_demod_trace_len(self._h, int(channel))
        arr = (WorkResult * n)()
        if n:
            check(self._lib.lorahip_demod_get_trace(self._h, int(channel), arr, n), "lorahip_demod_get_trace")
        return [dict((f, getattr(r, f)) for f, _ in WorkResult._fields_) for r in arr]


def _table_args(table):
    """(pointer, entries) of an optional (T,) int32 device table"""
    return _dptr(table), 0 if table is None else int(table.numel())


def _index_ok(index, table, P, rows_ok=True):
    import torch
    if index.dtype != torch.int32 or index.numel() != P or not rows_ok or (table is not None and table.dtype != torch.int32):
        raise ValueError("index must be (P,) int32, table (T,) int32 device tensors")


def _decode_rows(ctx, cfgs, n_cfgs, rows, nsyms, index, table, info, soft=False, width=None):
    """the one decoder call of LoRaDecoder (index None) and LoRaDecoderSet: checks, outputs, the entry point on the torch stream ->
    (out, out_len, dropped), and the (P, 8) header report with info. rows: (P, stride) 16-bit symbols (lorahip_decode_packets_info), or
    with soft (P, stride, W) float32 LLRs as Context.soft_symbols returns them (lorahip_decode_packets_soft, rows of stride * W floats); width: the
    W a single decoder reads -- a wider or narrower tensor is refused, not read as packed rows."""
    import torch
    if soft:
        if rows.dim() != 3 or rows.dtype != torch.float32 or nsyms.dtype != torch.int32:
            raise ValueError("llr must be (P, sym_stride, ppm) float32, nsyms (P,) int32 device tensors")
        if width is not None and int(rows.shape[2]) != width:
            raise ValueError("llr holds %d values per symbol, this decoder reads %d" % (int(rows.shape[2]), width))
    elif rows.dim() != 2 or rows.dtype not in (torch.int16, torch.uint16) or nsyms.dtype != torch.int32:
        raise ValueError("syms must be (P, stride) 16-bit, nsyms (P,) int32 device tensors")
    P, stride = int(rows.shape[0]), int(rows.shape[1])
    if index is not None:
        _index_ok(index, table, P, nsyms.numel() == P)
        index, table = index.contiguous(), None if table is None else table.contiguous()
    rows, nsyms = rows.contiguous(), nsyms.contiguous()
    out_stride = 2 * (stride + 8)
    out = torch.zeros((P, out_stride), dtype=torch.uint8, device=rows.device)
    out_len = torch.empty(P, dtype=torch.int32, device=rows.device)
    dropped = torch.empty(P, dtype=torch.int32, device=rows.device)
    rep = torch.empty((P, 8), dtype=torch.int32, device=rows.device) if info else None
    ctx.use_torch_stream()
    name = "lorahip_decode_packets_soft" if soft else "lorahip_decode_packets_info"
    row_args = (_dptr(rows), stride * int(rows.shape[2]), stride) if soft else (_dptr(rows), stride)
    check(getattr(ctx._lib, name)(ctx._h, cfgs, n_cfgs, _dptr(index), *_table_args(table), *row_args, _dptr(nsyms), P,
                                  _dptr(out), out_stride, _dptr(out_len), _dptr(dropped), _dptr(rep)), name)
    return (out, out_len, dropped, rep) if info else (out, out_len, dropped)


def _encode_rows(ctx, cfgs, n_cfgs, data, nbytes, index, table, sym_stride):
    """the one encoder call of LoRaEncoder (index None: lorahip_encode_packets) and LoRaEncoderSet (lorahip_encode_packets_cfgs): checks,
    outputs, the call on the torch stream -> (syms, nsyms)"""
    import torch
    if data.dim() != 2 or data.dtype != torch.uint8 or nbytes.dtype != torch.int32 or nbytes.numel() != data.shape[0]:
        raise ValueError("data must be a (P, stride) uint8, nbytes a (P,) int32 device tensor")
    P, stride = int(data.shape[0]), int(data.shape[1])
    if index is not None:
        _index_ok(index, table, P)
        index, table = index.contiguous(), None if table is None else table.contiguous()
    data, nbytes = data.contiguous(), nbytes.contiguous()
    syms = torch.empty((P, int(sym_stride)), dtype=torch.int16, device=data.device)
    nsyms = torch.empty(P, dtype=torch.int32, device=data.device)
    ctx.use_torch_stream()
    rows = (C.c_void_p(data.data_ptr()), stride, _dptr(nbytes), P, _dptr(syms), int(sym_stride), _dptr(nsyms))
    if index is None:
        check(ctx._lib.lorahip_encode_packets(ctx._h, cfgs, *rows), "lorahip_encode_packets")
    else:
        check(ctx._lib.lorahip_encode_packets_cfgs(ctx._h, cfgs, n_cfgs, _dptr(index), *_table_args(table), *rows), "lorahip_encode_packets_cfgs")
    return syms, nsyms


def _pack_symbols(packets):
    """list of symbol arrays -> ((P, stride) uint16 rows, stride at least 8, and (P,) int32 counts)"""
    host = np.zeros((len(packets), max(8, max(len(p) for p in packets))), np.uint16)
    for i, p in enumerate(packets):
        host[i, :len(p)] = np.asarray(p).astype(np.uint16)
    return host, np.array([len(p) for p in packets], np.int32)


def _decoded(out, out_len, interleaving):
    """the result list of a decoder's work(): a row's bytes (16-bit words without the de-interleaver: interleaving[i] false), None where
    the block posts nothing"""
    return [None if out_len[i] < 0 else out[i, :out_len[i]].copy() if interleaving[i] else out[i, :2 * out_len[i]].view(np.uint16).copy()
            for i in range(len(out_len))]


class LoRaDecoder:
    """The `/lora/lora_decoder` block (LoRaDecoder.cpp), same setters and defaults, for batches of symbol packets.

    work(packets): list of int16/uint16 symbol arrays (what LoRaDemod posts) -> list of bytes arrays (None where the
    block posts nothing); decode_batch(): the same on device tensors."""

    _CR = {"4/4": 0, "4/5": 1, "4/6": 2, "4/7": 3, "4/8": 4}      # the block's five strings (shared with LoRaEncoder)

    def __init__(self, device=0):
        self._ctx = Context(7, device=device)             # device + stream only; the decoder has its own sf
        self._cfg = DecoderCfg(C.sizeof(DecoderCfg), 10, 0, 4, 0, 1, 0, 1, 0, 8)   # LoRaDecoder.cpp:98-110
        self._whitening = True
        self._dropped = 0

    @staticmethod
    def make():
        return LoRaDecoder()

    def setSpreadFactor(self, sf): self._cfg.sf = int(sf)
    def setSymbolSize(self, ppm): self._cfg.ppm = int(ppm)

    def setCodingRate(self, cr):
        """one of the block's five strings, or "header" (the decoder only, not the block's): each packet at the rate its own explicit
        header names (LORAHIP_RDD_FROM_HEADER)"""
        if cr == "header":
            self._cfg.rdd = _lib.RDD_FROM_HEADER
            return
        if cr not in self._CR:
            raise ValueError("LoRaDecoder::setCodingRate(%s): unknown coding rate" % cr)   # InvalidArgumentException :150
        self._cfg.rdd = self._CR[cr]

    def enableWhitening(self, on): self._whitening = bool(on)     # stored, never read by work() -- like the reference
    def enableCrcc(self, on): self._cfg.crcc = int(bool(on))
    def enableInterleaving(self, on): self._cfg.interleaving = int(bool(on))
    def enableExplicit(self, on): self._cfg.explicit_hdr = int(bool(on))
    def enableHdr(self, on): self._cfg.hdr = int(bool(on))
    def enableErrorCheck(self, on): self._cfg.error_check = int(bool(on))
    def setDataLength(self, n): self._cfg.data_length = int(n)
    def getDropped(self): return self._dropped
    def activate(self): self._dropped = 0

    def decode_batch(self, syms, nsyms, info=False):
        """syms: (P, stride) int16/uint16 device tensor, nsyms: (P,) int32 device tensor ->
        (out uint8 (P, out_stride), out_len int32 (P,), dropped int32 (P,)) device tensors; info=True: a fourth, (P, 8) int32 -- the
        header report, a row per packet with the fields of struct lorahip_packet_info in include/lorahip.h"""
        return _decode_rows(self._ctx, C.byref(self._cfg), 1, syms, nsyms, None, None, info)

    def decode_soft(self, llr, nsyms, info=False):
        """decode_batch on rows of per-bit LLRs (Context.soft_symbols): llr (P, sym_stride, ppm) float32 with ppm this decoder's symbol
        size, nsyms (P,) int32 -> what decode_batch returns. Maximum-likelihood FEC nibbles; drops and the report as the hard decoder's
        (lorahip_decode_packets_soft in include/lorahip.h). Needs the de-interleaver on."""
        return _decode_rows(self._ctx, C.byref(self._cfg), 1, llr, nsyms, None, None, info, soft=True, width=self._cfg.ppm or self._cfg.sf)

    def work(self, packets):
        import torch
        if self._cfg.ppm > self._cfg.sf:
            raise ValueError("LoRaDecoder::work(): failed check: PPM <= SF")            # Pothos::Exception :202
        P = len(packets)
        if P == 0:
            return []
        host, n = _pack_symbols(packets)
        dev = torch.device("cuda", self._ctx.device)
        out, out_len, dropped = self.decode_batch(torch.from_numpy(host.view(np.int16)).to(dev), torch.from_numpy(n).to(dev))
        out, out_len, dropped = out.cpu().numpy(), out_len.cpu().numpy(), dropped.cpu().numpy()
        self._dropped += int(dropped.sum())
        return _decoded(out, out_len, [self._cfg.interleaving] * P)


class LoRaDecoderSet:
    """1..64 configured LoRaDecoder objects as ONE launch whose packets each pick their decoder (lorahip_decode_packets_cfgs): the
    decoder of a receiver over several SFs and coding rates. The configurations are copied at construction (later setter calls on
    the decoders do not reach the set). Packet p is decoded exactly as decoders[i].decode_batch would decode it, i = index[p], or
    table[index[p]] with a table (index = the channels LoRaDemod.packets_device() returns, table = decoder of channel); out_len is -3
    where there is no such decoder. One launch has one LDS slice per packet, the largest any member needs: a member without a
    header and with a data length of thousands of bytes slows every packet of the launch (LoRaDecoderSet.plan)."""

    def __init__(self, decoders, device=0):
        decoders = list(decoders)
        if not 1 <= len(decoders) <= 64:
            raise ValueError("LoRaDecoderSet: 1..64 decoders")
        self._ctx = Context(7, device=device)             # device + stream only
        self._cfgs = self._table(decoders)
        self._dropped = 0

    @staticmethod
    def _table(decoders):
        cfgs = (DecoderCfg * len(decoders))()
        for i, d in enumerate(decoders):
            C.memmove(C.byref(cfgs[i]), C.byref(d._cfg), C.sizeof(DecoderCfg))
        return cfgs

    @staticmethod
    def plan(decoders, sym_stride):
        """what a launch of these decoders over rows of sym_stride symbols runs on (lorahip_decode_plan; no device needed): a dict with
        the fields of struct lorahip_decode_tiling in include/lorahip.h. Raises LoraHipError where decode_batch would."""
        decoders = list(decoders)
        cfgs = LoRaDecoderSet._table(decoders) if decoders else None
        t = _lib.DecodeTiling(C.sizeof(_lib.DecodeTiling))
        check(load().lorahip_decode_plan(cfgs, len(decoders), int(sym_stride), C.byref(t)), "lorahip_decode_plan")
        return dict((f, int(getattr(t, f))) for f, _ in _lib.DecodeTiling._fields_ if f not in ("struct_size", "reserved"))

    def getDropped(self): return self._dropped
    def activate(self): self._dropped = 0

    def decode_batch(self, syms, nsyms, index, table=None, info=False):
        """syms: (P, stride) int16/uint16, nsyms: (P,) int32, index: (P,) int32, table: (T,) int32 or None -- device tensors ->
        (out uint8 (P, out_stride), out_len int32 (P,), dropped int32 (P,)) device tensors, as LoRaDecoder.decode_batch (info=True: and the
        (P, 8) int32 header report)"""
        return _decode_rows(self._ctx, self._cfgs, len(self._cfgs), syms, nsyms, index, table, info)

    def decode_soft(self, llr, nsyms, index, table=None, info=False):
        """decode_batch on rows of per-bit LLRs, as LoRaDecoder.decode_soft: llr (P, sym_stride, W) float32; a packet whose decoder reads
        ppm < W bits per symbol has its symbol s at s * ppm of its row (lorahip_decode_packets_soft)"""
        return _decode_rows(self._ctx, self._cfgs, len(self._cfgs), llr, nsyms, index, table, info, soft=True)

    def work(self, packets, index):
        """list of symbol arrays and the decoder of each -> list of bytes arrays (None where the block posts nothing), as
        LoRaDecoder.work; raises where a packet has no decoder (-3) or does not fit the rows (-2)"""
        import torch
        P = len(packets)
        if len(index) != P:
            raise ValueError("LoRaDecoderSet.work(): one index per packet")
        if P == 0:
            return []
        host, n = _pack_symbols(packets)
        idx = np.asarray(index, np.int64)
        dev = torch.device("cuda", self._ctx.device)
        out, out_len, dropped = self.decode_batch(torch.from_numpy(host.view(np.int16)).to(dev), torch.from_numpy(n).to(dev),
                                                  torch.from_numpy(np.clip(idx, -1, 2 ** 31 - 1).astype(np.int32)).to(dev))
        out, out_len, dropped = out.cpu().numpy(), out_len.cpu().numpy(), dropped.cpu().numpy()
        self._dropped += int(dropped.sum())
        for i in range(P):
            if out_len[i] == -3:
                raise ValueError("LoRaDecoderSet.work(): packet %d names decoder %d of %d" % (i, int(idx[i]), len(self._cfgs)))
            if out_len[i] == -2:
                raise ValueError("LoRaDecoderSet.work(): packet %d does not fit its row" % i)
        return _decoded(out, out_len, [self._cfgs[int(j)].interleaving for j in idx])


class LoRaEncoder:
    """The `/lora/lora_encoder` block (LoRaEncoder.cpp), same setters and defaults, for batches of byte messages of different lengths.

    work(messages): list of bytes-like -> list of uint16 symbol arrays (None where the block has no defined result: an empty message
    without crc and header); encode_batch(): the same on device tensors. Pad nibbles are 0 (include/lorahip.h)."""

    _CR = LoRaDecoder._CR

    def __init__(self, device=0, ctx=None):
        self._ctx = ctx if ctx is not None else Context(7, device=device)   # device + stream only; the encoder has its own sf
        self._cfg = EncoderCfg(C.sizeof(EncoderCfg), 10, 0, 4, 1, 1, 1)    # LoRaEncoder.cpp:78-85

    @staticmethod
    def make():
        return LoRaEncoder()

    def setSpreadFactor(self, sf): self._cfg.sf = int(sf)
    def setSymbolSize(self, ppm): self._cfg.ppm = int(ppm)

    def setCodingRate(self, cr):
        if cr not in self._CR:
            raise ValueError("LoRaEncoder::setCodingRate(%s): unknown coding rate" % cr)   # InvalidArgumentException :118
        self._cfg.rdd = self._CR[cr]

    def enableWhitening(self, on): self._cfg.whitening = int(bool(on))
    def enableExplicit(self, on): self._cfg.explicit_hdr = int(bool(on))
    def enableCrc(self, on): self._cfg.crc = int(bool(on))

    def num_symbols(self, n_bytes):
        """symbols of a message of n_bytes bytes (host arithmetic); -1 where nothing is defined or the configuration is refused"""
        return int(self._ctx._lib.lorahip_encode_num_symbols(C.byref(self._cfg), int(n_bytes)))

    def encode_batch(self, data, nbytes, sym_stride=None):
        """data: (P, stride) uint8 device tensor, nbytes: (P,) int32 device tensor -> (syms uint16-as-int16 (P, sym_stride), nsyms int32
        (P,)) device tensors, queued on the torch stream. sym_stride defaults to what a message of `stride` bytes needs."""
        if sym_stride is None and data.dim() == 2:
            sym_stride = max(8, self.num_symbols(min(int(data.shape[1]), self._ctx._lib.lorahip_encode_max_bytes())))
        return _encode_rows(self._ctx, C.byref(self._cfg), 1, data, nbytes, None, None, sym_stride)

    def work(self, messages):
        import torch
        if self._cfg.ppm > self._cfg.sf:
            raise ValueError("LoRaEncoder::work(): failed check: PPM <= SF")            # Pothos::Exception :166
        P = len(messages)
        if P == 0:
            return []
        host, n = _pack_rows(messages)
        dev = torch.device("cuda", self._ctx.device)
        syms, nsyms = self.encode_batch(torch.from_numpy(host).to(dev), torch.from_numpy(n).to(dev))
        syms, nsyms = syms.cpu().numpy().view(np.uint16), nsyms.cpu().numpy()
        if (nsyms == -2).any():
            raise ValueError("LoRaEncoder.work(): a message is longer than this build encodes (lorahip_encode_max_bytes())")
        return [syms[i, :nsyms[i]].copy() if nsyms[i] >= 0 else None for i in range(P)]


def _pack_rows(messages):
    """list of bytes-like -> ((P, stride) uint8 rows, (P,) int32 lengths)"""
    arrs = [np.frombuffer(bytes(m), np.uint8) if isinstance(m, (bytes, bytearray, memoryview)) else np.asarray(m).astype(np.uint8).reshape(-1)
            for m in messages]
    host = np.zeros((len(arrs), max(1, max(a.size for a in arrs))), np.uint8)
    for i, a in enumerate(arrs):
        host[i, :a.size] = a
    return host, np.array([a.size for a in arrs], np.int32)


def transmit(payloads, sf=10, cr="4/8", sync=0x12, ampl=1.0, padding=1, sigma=0.0, seed=0, nbytes=None, ppm=0, explicit=True, crc=True,
             whitening=True, lead=0, tail=0, ctx=None, device=0):
    """bytes -> symbols -> IQ -> (noise) on the device, for messages of different lengths: LoRaEncoder.encode_batch ->
    Context.mod_frames(nsyms=) -> Context.add_awgn, all queued on the torch stream with no host synchronisation in between.

    payloads: a list of bytes-like, or a (P, stride) uint8 device tensor with nbytes a (P,) int32 device tensor.
    ctx: a Context(sf) to reuse (one is made and closed otherwise). Returns (iq (P, lead + frame + tail) complex64, nsyms (P,) int32):
    every row has the length of the longest message `stride` bytes can make; a refused message (nsyms < 0) gives a silent row."""
    import torch
    own = ctx is None
    if own:
        ctx = Context(sf, device=device)
    elif ctx.sf != int(sf):
        raise ValueError("ctx is a Context of SF%d, not SF%d" % (ctx.sf, sf))
    try:
        if not _is_torch(payloads):
            host, n = _pack_rows(payloads)
            dev = torch.device("cuda", ctx.device)
            payloads, nbytes = torch.from_numpy(host).to(dev), torch.from_numpy(n).to(dev)
        elif nbytes is None:
            raise ValueError("device payload rows need nbytes, a (P,) int32 device tensor")
        enc = LoRaEncoder(ctx=ctx)
        enc.setSpreadFactor(sf); enc.setSymbolSize(ppm); enc.setCodingRate(cr)
        enc.enableExplicit(explicit); enc.enableCrc(crc); enc.enableWhitening(whitening)
        syms, nsyms = enc.encode_batch(payloads, nbytes)
        iq = ctx.mod_frames(syms, sync=sync, ampl=ampl, padding=padding, lead=lead, tail=tail, nsyms=nsyms)
        if sigma:
            ctx.add_awgn(iq, sigma, seed)
        if own:
            ctx.synchronize()                  # the context's tables must outlive the queued work
        return iq, nsyms
    finally:
        if own:
            ctx.close()


class LoRaEncoderSet:
    """1..64 configured LoRaEncoder objects as ONE launch whose packets each pick their encoder (lorahip_encode_packets_cfgs): the
    encoder of a transmitter over several SFs and coding rates, the mirror of LoRaDecoderSet. The configurations are copied at
    construction (later setter calls on the encoders do not reach the set). Packet p is encoded exactly as encoders[i].encode_batch
    would encode it, i = index[p], or table[index[p]] with a table; nsyms is -3 and the row zero where there is no such encoder."""

    def __init__(self, encoders, device=0, ctx=None):
        encoders = list(encoders)
        if not 1 <= len(encoders) <= 64:
            raise ValueError("LoRaEncoderSet: 1..64 encoders")
        self._ctx = ctx if ctx is not None else Context(7, device=device)   # device + stream only
        self._cfgs = (EncoderCfg * len(encoders))()
        for i, e in enumerate(encoders):
            C.memmove(C.byref(self._cfgs[i]), C.byref(e._cfg), C.sizeof(EncoderCfg))

    def __len__(self):
        return len(self._cfgs)

    def _on(self, ctx):
        """the same table launched through another context (its device and stream)"""
        other = LoRaEncoderSet.__new__(LoRaEncoderSet)
        other._ctx, other._cfgs = ctx, self._cfgs
        return other

    @property
    def spread_factors(self):
        """the SF of every member, in order"""
        return [int(c.sf) for c in self._cfgs]

    def num_symbols(self, i, n_bytes):
        """symbols of a message of n_bytes bytes under member i (host arithmetic), as LoRaEncoder.num_symbols"""
        return int(self._ctx._lib.lorahip_encode_num_symbols(C.byref(self._cfgs[int(i)]), int(n_bytes)))

    def max_symbols(self, n_bytes):
        """the largest num_symbols(i, n_bytes) over the members (at least 8): the symbol stride that holds any message of n_bytes bytes"""
        return max(8, max(self.num_symbols(i, n_bytes) for i in range(len(self._cfgs))))

    def encode_batch(self, data, nbytes, index, table=None, sym_stride=None):
        """data: (P, stride) uint8, nbytes: (P,) int32, index: (P,) int32, table: (T,) int32 or None -- device tensors -> (syms
        uint16-as-int16 (P, sym_stride), nsyms int32 (P,)) device tensors, queued on the torch stream. sym_stride defaults to what a
        message of `stride` bytes needs under the member that makes most of it."""
        if sym_stride is None and data.dim() == 2:
            sym_stride = self.max_symbols(min(int(data.shape[1]), self._ctx._lib.lorahip_encode_max_bytes()))
        return _encode_rows(self._ctx, self._cfgs, len(self._cfgs), data, nbytes, index, table, sym_stride)

    def work(self, messages, index):
        """list of bytes-like and the encoder of each -> list of uint16 symbol arrays (None where the block has no defined result), as
        LoRaEncoder.work; raises where a message has no encoder (-3) or is longer than this build encodes (-2)"""
        import torch
        P = len(messages)
        if len(index) != P:
            raise ValueError("LoRaEncoderSet.work(): one index per message")
        if P == 0:
            return []
        host, n = _pack_rows(messages)
        idx = np.asarray(index, np.int64)
        dev = torch.device("cuda", self._ctx.device)
        syms, nsyms = self.encode_batch(torch.from_numpy(host).to(dev), torch.from_numpy(n).to(dev),
                                        torch.from_numpy(np.clip(idx, -1, 2 ** 31 - 1).astype(np.int32)).to(dev))
        syms, nsyms = syms.cpu().numpy().view(np.uint16), nsyms.cpu().numpy()
        for i in range(P):
            if nsyms[i] == -3:
                raise ValueError("LoRaEncoderSet.work(): message %d names encoder %d of %d" % (i, int(idx[i]), len(self._cfgs)))
            if nsyms[i] == -2:
                raise ValueError("LoRaEncoderSet.work(): message %d is longer than this build encodes (lorahip_encode_max_bytes())" % i)
        return [syms[i, :nsyms[i]].copy() if nsyms[i] >= 0 else None for i in range(P)]


def _to_dev(x, dtype, dev):
    """a device tensor of `dtype` from a device tensor, an array or a list"""
    import torch
    if _is_torch(x):
        return x.to(device=dev, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.dtype(str(dtype).replace("torch.", "")))).to(dev)


def transmit_mixed(payloads, encoders, index, row, start, n_rows, row_len, table=None, sync=0x12, ampl=1.0, sigma=0.0, seed=0, nbytes=None,
                   out=None, ctx=None, device=0):
    """bytes -> symbols -> IQ -> (noise) on the device for frames of DIFFERENT SF and coding rate placed in channel rows: ONE
    LoRaEncoderSet.encode_batch -> ONE Context.mod_frames_sched -> Context.add_awgn, all queued on the torch stream with no host
    synchronisation in between -- a downlink scheduler, or the load in front of a synthesiser or a mixed-SF receiver.

    payloads: a list of bytes-like, or a (P, stride) uint8 device tensor with nbytes a (P,) int32 device tensor.
    encoders: 1..64 LoRaEncoder objects, or a LoRaEncoderSet. Frame p is encoded by encoders[i], i = index[p] or table[index[p]], and
    modulated at THAT encoder's SF (gathered on the device) into out[row[p], start[p]:start[p] + body] (lorahip_mod_body_len). index, row
    (int32), start (int64) and table: device tensors, arrays or lists. Frames must not overlap; the rest of the rows is silence.
    out: a contiguous (n_rows, row_len) complex64 device tensor to write into (it is zeroed first), or None to make one.
    ctx: any Context to reuse (device and stream only; one is made and closed otherwise).
    Returns (iq (n_rows, row_len) complex64, nsyms (P,) int32, status (P,) int32): status as Context.mod_frames_sched -- a message without
    an encoder (nsyms -3) or refused by it (-1, -2) has status -1 and its slot stays silent."""
    import torch
    own = ctx is None
    if own:
        ctx = Context(7, device=device)
    try:
        dev = torch.device("cuda", ctx.device)
        if not _is_torch(payloads):
            host, n = _pack_rows(payloads)
            payloads, nbytes = torch.from_numpy(host).to(dev), torch.from_numpy(n).to(dev)
        elif nbytes is None:
            raise ValueError("device payload rows need nbytes, a (P,) int32 device tensor")
        encs = encoders._on(ctx) if isinstance(encoders, LoRaEncoderSet) else LoRaEncoderSet(encoders, ctx=ctx)
        index, row, start = _to_dev(index, torch.int32, dev), _to_dev(row, torch.int32, dev), _to_dev(start, torch.int64, dev)
        table = None if table is None else _to_dev(table, torch.int32, dev)
        if out is None:
            out = torch.zeros((int(n_rows), int(row_len)), dtype=torch.complex64, device=dev)
        else:
            if tuple(out.shape) != (int(n_rows), int(row_len)) or out.dtype != torch.complex64 or not out.is_contiguous():
                raise ValueError("out must be a contiguous (n_rows, row_len) complex64 device tensor")
            out.zero_()
        stride = min(int(payloads.shape[1]), ctx._lib.lorahip_encode_max_bytes())
        syms, nsyms = encs.encode_batch(payloads, nbytes, index, table=table, sym_stride=encs.max_symbols(stride))
        # the SF of every frame: that of its encoder, 0 (no such SF) where it has none -- gathered on the device
        sf_of = torch.tensor(encs.spread_factors, dtype=torch.int32, device=dev)
        i = index.to(torch.int64)
        if table is not None:
            ok = (i >= 0) & (i < table.numel())
            i = torch.where(ok, table.to(torch.int64)[i.clamp(0, table.numel() - 1)], torch.full_like(i, -1))
        ok = (i >= 0) & (i < sf_of.numel())
        sf = torch.where(ok, sf_of[i.clamp(0, sf_of.numel() - 1)], torch.zeros((), dtype=torch.int32, device=dev)).contiguous()
        status = ctx.mod_frames_sched(syms, nsyms, sf, row, start, out, ampl=ampl, sync=sync)
        if sigma:
            ctx.add_awgn(out, sigma, seed)
        if own:
            ctx.synchronize()                  # the context must outlive the queued work
        return out, nsyms, status
    finally:
        if own:
            ctx.close()


def match_signals(info, chan, sig_chan, sig_pos):
    """Which signal belongs to which packet: per packet the index of its signal in (sig_chan, sig_pos), or -1 where there is none, by
    the exact key (channel, sync_pos) == (signal channel, signal position) -- a frame's signals are emitted by its DOWNCHIRP1 call,
    whose start is the packet's sync_pos (lorahip_rx_info). info: (P, 4) int64 as packets_arrays / packets_device / receiver_rows
    (info=True) give it; chan: (P,); sig_chan, sig_pos: (S,) as signals(pos=True) / receiver_signal_rows(pos=True) give them -- all
    numpy arrays, or all device tensors: then the (P,) int64 result is a device tensor and nothing is synchronised with the host (every
    shape follows from the arguments' shapes). Compared in blocks of at most 2^22 pairs."""
    if not _is_torch(info):
        info, sig_pos = np.asarray(info, np.int64).reshape(-1, 4), np.asarray(sig_pos, np.int64)
    P, S = int(info.shape[0]), int(sig_pos.shape[0])
    if _is_torch(info):
        import torch
        out = torch.full((P,), -1, dtype=torch.int64, device=info.device)
        if P == 0 or S == 0:
            return out
        sync, ch, sch, sps = info[:, 2], chan.to(torch.int64), sig_chan.to(torch.int64), sig_pos.to(torch.int64)
        step = max(1, (1 << 22) // S)
        for p0 in range(0, P, step):
            hit = (ch[p0:p0 + step, None] == sch[None, :]) & (sync[p0:p0 + step, None] == sps[None, :])
            out[p0:p0 + step] = torch.where(hit.any(1), hit.to(torch.int8).argmax(1), out[p0:p0 + step])
        return out
    ch, sch, sps = np.asarray(chan, np.int64), np.asarray(sig_chan, np.int64), sig_pos
    out = np.full(P, -1, np.int64)
    if P == 0 or S == 0:
        return out
    step = max(1, (1 << 22) // S)
    for p0 in range(0, P, step):
        hit = (ch[p0:p0 + step, None] == sch[None, :]) & (info[p0:p0 + step, 2, None] == sps[None, :])
        out[p0:p0 + step] = np.where(hit.any(1), hit.argmax(1), -1)
    return out
