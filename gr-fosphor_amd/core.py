"""Host-side mirror of the reference's libfosphor interface over the HIP library.

Same names and argument meaning as lib/fosphor/fosphor.h (process / draw / set_fft_window /
set_power_range / set_frequency_range) plus the plain-buffer accessors that replace the
CL<->GL interop.  Everything numeric happens in libfosphor_amd.so on the GPU; this class
only marshals pointers.
"""
import ctypes as C
import errno

import numpy as np

from . import _lib

FFT_LEN_LOG = 10		# private.h:21
FFT_LEN = 1 << FFT_LEN_LOG
MULT_BATCH = 16			# private.h:24
MAX_BATCH = 1024		# private.h:25


IQ_FORMATS = {"fp32": 0, "fp16": 1, "sc16": 2}	# FOSPHOR_AMD_IQ_* (include/fosphor_amd.h)
WIRE_FORMS = {"packed16": 1, "sparse16": 2}	# FOSPHOR_AMD_WIRE_* (include/fosphor_amd_wire.h)
WIRE_MAX_BATCH = 65535


K1_KERNELS = ("k1_fft_bin", "k1v2_fft_bin", "k1big_fft_bin", "k1w_fft_bin", "k1h_fused")	# FOSPHOR_AMD_K1_* (include/fosphor_amd.h)


def plan_k1(fft_len_log, n_bins, iq_format, hop, iq_align, total, batch, tile_knob=0, k1_knob=1, n_cus=256):
    """fosphor_amd_plan_k1 (host arithmetic, no device): the FFT launch of one piece of `total` spectra in batches of `batch` as a
    dict -- kernel (a K1_KERNELS name), tile, tiles, units, max_tiles, min_tiles.  iq_format: "fp32" / "fp16" / "sc16" or a
    FOSPHOR_AMD_IQ_* number; hop: samples between spectrum starts; iq_align: byte address of the first sample (modulo 16 is what
    counts); tile_knob / k1_knob: the FOSPHOR_AMD_TILE / FOSPHOR_AMD_K1 settings the instance was made under."""
    fmt = IQ_FORMATS[iq_format] if isinstance(iq_format, str) else int(iq_format)
    p = _lib.K1Plan()
    rv = _lib.load().fosphor_amd_plan_k1(fft_len_log, n_bins, fmt, hop, int(iq_align) & 15, tile_knob, k1_knob, n_cus, total, batch,
                                         C.byref(p))
    if rv:
        _fail("fosphor_amd_plan_k1", rv, ValueError)
    out = {k: getattr(p, k) for k, _ in _lib.K1Plan._fields_}
    out["kernel"] = K1_KERNELS[p.kernel]
    return out


def _ptr(x):
    """Device pointer of a torch tensor / anything with data_ptr(), or a raw integer."""
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


def _fail(name, rv, exc):
    """the library's `name` returned rv"""
    raise exc("%s -> %d (%s)" % (name, rv, errno.errorcode.get(-rv, "?")))


def _iq_count(x, n, name, floats=True):
    """Samples of the device IQ x: n where given (a raw pointer needs it), else from the tensor, which must be contiguous and,
    with floats, complex64 or float32 pairs"""
    if n is not None:
        return int(n)
    if not hasattr(x, "numel"):
        raise ValueError("a raw device pointer needs %s" % ("n_samples" if name == "d_iq" else "n_" + name))
    if not floats:
        if not x.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    elif not x.is_contiguous() or str(x.dtype) not in ("torch.complex64", "torch.float32"):
        raise ValueError("%s must be a contiguous complex64 or float32 tensor" % name)
    return x.numel() if x.is_complex() else x.numel() // 2


def _float_pairs(x):
    """complex64 or float32 pairs on the host -> flat float32"""
    x = np.ascontiguousarray(x)
    x = x.view(np.float32) if x.dtype == np.complex64 else np.ascontiguousarray(x, dtype=np.float32)
    return x.reshape(-1)


def _or_dummy(x):
    """x, or something to point at when there are no samples (the caller holds it for as long as the pointer is in use)"""
    return x if x.size else np.zeros(2, np.float32)


def _outs(jobs, n_out_fn):
    """(n_out per job, the capacity the jobs need)"""
    n_out = [n_out_fn(j) for j in jobs]
    return n_out, max([int(j["out_offset"]) + n for j, n in zip(jobs, n_out)] + [0])


def _check_f32(t, n, what, message="%s must be a contiguous float32 device tensor of %d elements"):
    """t is a contiguous float32 device tensor of n elements, or ValueError(message % (what, n))"""
    if str(t.dtype) != "torch.float32" or t.numel() != n or not t.is_cuda or not t.is_contiguous():
        raise ValueError(message % (what, n))


def _result(d_res, Struct):
    """a result struct on the device -> dict"""
    r = Struct.from_buffer_copy(d_res.cpu().numpy().tobytes())
    return {k: getattr(r, k) for k, _ in Struct._fields_}


class Fosphor:
    """One fosphor instance (struct fosphor).  Reference geometry by default."""

    def __init__(self, n_bins=128, wf_rows=1024, fft_len_log=FFT_LEN_LOG, t0r=0.0, t0d=0.0, alpha=0.0,
                 device=-1, max_spectra=1024, max_batches=0, stream=None, iq_fp16=False, iq_format=None):
        """iq_format: "fp32" (default), "fp16" (fft_len_log 16 only; iq_fp16=True says the same) or "sc16" (interleaved
        int16, value i * 2**-15) -- or the FOSPHOR_AMD_IQ_* number; the library refuses formats it does not know."""
        self.L = _lib.load()
        if iq_format is None:
            fmt = 1 if iq_fp16 else 0
        elif isinstance(iq_format, str):
            if iq_format not in IQ_FORMATS:
                raise ValueError("iq_format must be one of %s" % ", ".join(IQ_FORMATS))
            fmt = IQ_FORMATS[iq_format]
        else:
            fmt = int(iq_format)
        if iq_fp16 and fmt != 1:
            raise ValueError("iq_fp16=True contradicts iq_format=%r" % (iq_format,))
        cfg = _lib.Config(fft_len_log, n_bins, wf_rows, t0r, t0d, alpha, device, max_spectra, max_batches,
                          C.c_void_p(stream) if stream else None, fmt)
        self.iq_format = fmt
        self.iq_fp16 = fmt == 1
        self.iq_sc16 = fmt == 2
        self.h = self.L.fosphor_amd_init(C.byref(cfg))
        if not self.h:
            raise RuntimeError("fosphor_amd_init failed (see stderr); no CPU fallback exists")
        self.n, self.n_bins, self.wf_rows = 1 << fft_len_log, n_bins, wf_rows
        self.max_spectra = max_spectra

    def close(self):
        if getattr(self, "h", None):
            self.L.fosphor_release(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _window(self, first_bin, n_cols, rows=None, most_rows=None):
        """(n_cols, rows) of a window with the defaults filled in: every column from first_bin on, every waterfall row (at most
        most_rows of them)"""
        if n_cols is None:
            n_cols = self.n - first_bin
        if rows is None:
            rows = self.wf_rows if most_rows is None else min(self.wf_rows, most_rows)
        return n_cols, rows

    def _stats(self, fn, names):
        """the counters a fosphor_amd_*_stats copies, as a dict"""
        st = (C.c_longlong * len(names))()
        rv = fn(self.h, C.byref(st))
        if rv:
            raise RuntimeError("%s -> %d" % (fn.__name__, rv))
        return dict(zip(names, list(st)))

    # ---- reference API ---------------------------------------------------
    def process(self, samples):
        """fosphor_process: host interleaved (re, im) in the instance's format -- fp32 (fp16); on sc16 instances an int16 numpy
        array only, flat of even length or (n, 2) (TypeError otherwise: floats are never converted silently).
        Returns 0 / -EINVAL / -EIO."""
        if self.iq_sc16:
            if not isinstance(samples, np.ndarray) or samples.dtype != np.int16:
                raise TypeError("an sc16 instance takes an int16 numpy array, got %s" % getattr(samples, "dtype", type(samples).__name__))
            if not (samples.ndim == 1 and samples.size % 2 == 0) and not (samples.ndim == 2 and samples.shape[1] == 2):
                raise TypeError("sc16 samples must be flat (re, im, ...) of even length or of shape (n, 2), got %s" % (samples.shape,))
            x = np.ascontiguousarray(samples).reshape(-1)
        else:
            x = np.ascontiguousarray(samples, dtype=np.float16 if self.iq_fp16 else np.float32).reshape(-1)
        return self.L.fosphor_process(self.h, x.ctypes.data, x.size // 2)

    def draw(self, render=None):
        r = render if render is not None else _lib.Render()
        self.L.fosphor_draw(self.h, C.byref(r))
        return r._wf_pos

    def set_fft_window_default(self):
        self.L.fosphor_set_fft_window_default(self.h)

    def set_fft_window(self, win):
        w = np.ascontiguousarray(win, dtype=np.float32)
        if w.size != self.n:
            raise ValueError("window must have %d taps" % self.n)
        self.L.fosphor_set_fft_window(self.h, w.ctypes.data)

    def set_power_range(self, db_ref, db_per_div):
        self.L.fosphor_set_power_range(self.h, int(db_ref), int(db_per_div))

    def set_frequency_range(self, center, span):
        self.L.fosphor_set_frequency_range(self.h, float(center), float(span))

    # ---- device-resident data path -----------------------------------------
    def _dev(self, d_samples):
        """Device pointer of the samples; on sc16 instances a torch tensor must be int16 (ValueError otherwise)."""
        if self.iq_sc16 and hasattr(d_samples, "data_ptr") and hasattr(d_samples, "dtype") and str(d_samples.dtype) != "torch.int16":
            raise ValueError("an sc16 instance reads int16 samples, got a %s tensor" % d_samples.dtype)
        return _ptr(d_samples)

    def process_device(self, d_samples, n_batches, batch):
        return self.L.fosphor_amd_process_device(self.h, self._dev(d_samples), int(n_batches), int(batch))

    def process_device_overlap(self, d_samples, n_batches, batch, overlap):
        """overlap_cc(wlen=N, overlap) fused into the read (unexpanded stream in HBM)."""
        return self.L.fosphor_amd_process_device_overlap(self.h, self._dev(d_samples), int(n_batches), int(batch), int(overlap))

    def finish(self):
        return self.L.fosphor_amd_finish(self.h)

    def accumulate_device(self, d_samples, n_local, t_offset, total_batch, overlap=1):
        if overlap > 1:
            return self.L.fosphor_amd_accumulate_device_overlap(self.h, self._dev(d_samples), n_local, t_offset, total_batch, overlap)
        return self.L.fosphor_amd_accumulate_device(self.h, self._dev(d_samples), n_local, t_offset, total_batch)

    def merge(self, total_batch):
        return self.L.fosphor_amd_merge(self.h, total_batch)

    def set_partial_slot(self, slot):
        return self.L.fosphor_amd_set_partial_slot(self.h, slot)

    def partials(self):
        p = _lib.Partials()
        self.L.fosphor_amd_get_partials(self.h, C.byref(p))
        return p

    # ---- native exchange (RCCL, include/fosphor_amd.h) ------------------------
    def exchange(self, comm):
        return self.L.fosphor_amd_exchange(self.h, comm)

    def exchange_sliced(self, comm, world, rank):
        return self.L.fosphor_amd_exchange_sliced(self.h, comm, world, rank)

    def merge_sliced(self, total_batch, world, rank):
        return self.L.fosphor_amd_merge_sliced(self.h, total_batch, world, rank)

    def gather_state(self, comm, world, rank):
        return self.L.fosphor_amd_gather_state(self.h, comm, world, rank)

    # ---- compact wire formats of the exchange (include/fosphor_amd_wire.h) ----
    @staticmethod
    def _wire_form(form):
        """"packed16" / "sparse16" or the FOSPHOR_AMD_WIRE_* number (which the library checks)"""
        if isinstance(form, str):
            if form not in WIRE_FORMS:
                raise ValueError("wire form must be one of %s" % ", ".join(WIRE_FORMS))
            return WIRE_FORMS[form]
        return int(form)

    def wire_mask(self, total_batch, world, rank):
        """stage (a) of the sparse form: this rank's presence bits into its part of the mask buffer; 0 / -EINVAL / -EIO"""
        return self.L.fosphor_amd_wire_mask(self.h, int(total_batch), int(world), int(rank))

    def wire_pack(self, total_batch, form, world):
        """fosphor_amd_wire_pack: (return value, struct fosphor_amd_wire)"""
        w = _lib.Wire()
        rv = self.L.fosphor_amd_wire_pack(self.h, int(total_batch), self._wire_form(form), int(world), C.byref(w))
        return rv, w

    def wire_unpack(self):
        return self.L.fosphor_amd_wire_unpack(self.h)

    def wire_info(self):
        """struct fosphor_amd_wire as it stands: the buffers and what the last pack decided"""
        w = _lib.Wire()
        rv = self.L.fosphor_amd_wire_get(self.h, C.byref(w))
        if rv:
            raise RuntimeError("fosphor_amd_wire_get -> %d" % rv)
        return w

    def exchange_compact(self, comm, total_batch, form, world, rank):
        return self.L.fosphor_amd_exchange_compact(self.h, comm, int(total_batch), self._wire_form(form), int(world), int(rank))

    WIRE_STATS = ("packed16", "sparse16", "fell_back", "live_rows", "wire_bytes")

    def wire_stats(self):
        """fosphor_amd_wire_stats as a dict: packs since the instance was made by the form they took (WIRE_STATS[:3]), live rows
        and wire bytes (masks included) of the last one"""
        return self._stats(self.L.fosphor_amd_wire_stats, self.WIRE_STATS)

    def wire_kernel_times(self):
        """ms of the last k_wire_mask / k_wire_pack / k_wire_unpack launch made while profiling was on (-1: none)"""
        ms = (C.c_float * 3)()
        rv = self.L.fosphor_amd_wire_kernel_times(self.h, C.byref(ms))
        if rv:
            raise RuntimeError("fosphor_amd_wire_kernel_times -> %d" % rv)
        return dict(zip(("mask", "pack", "unpack"), list(ms)))

    def buffers(self, hitcount=True):
        """struct fosphor_amd_buffers; hitcount=False: no export kernel, no wait, d_hitcount is NULL."""
        b = _lib.Buffers()
        rv = (self.L.fosphor_amd_get_buffers if hitcount else self.L.fosphor_amd_get_buffers_nohc)(self.h, C.byref(b))
        if rv:
            raise RuntimeError("fosphor_amd_get_buffers -> %d" % rv)
        return b

    # ---- results as host arrays ------------------------------------------
    def _read(self, which, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        rv = self.L.fosphor_amd_read(self.h, which, out.ctypes.data, out.nbytes)
        if rv:
            raise RuntimeError("fosphor_amd_read(%d) -> %d (%s)" % (which, rv, errno.errorcode.get(-rv, "?")))
        return out

    @property
    def waterfall(self):
        return self._read(0, (self.wf_rows, self.n), np.float32)

    @property
    def histogram(self):
        return self._read(1, (self.n_bins, self.n), np.float32)

    @property
    def spectrum(self):
        return self._read(2, (2, self.n, 2), np.float32)

    @property
    def hitcount(self):
        """uint32 [n_bins][N] of the last batch (the oracle's view is the transpose)."""
        return self._read(3, (self.n_bins, self.n), np.uint32)

    @property
    def waterfall_pos(self):
        return self.buffers(False).waterfall_pos

    def colorize(self, image, palette=None, scale=None, offset=None, rows=None):
        """RGBA8 picture of the waterfall (image=0, newest row first) or the histogram (image=1,
        highest bin first), fft-shifted, as a torch uint8 tensor [rows][N][4] on the device.
        palette: numpy uint32[n] (host) or None for the reference's 256-entry palette of that image;
        scale/offset None: the reference's values (include/fosphor_amd_cmap.h)."""
        import torch
        if rows is None:
            rows = self.wf_rows if image == 0 else self.n_bins
        out = torch.empty((rows, self.n), dtype=torch.int32, device="cuda")
        if palette is not None:
            palette = np.ascontiguousarray(palette, dtype=np.uint32)
        defaults = scale is None and offset is None
        rv = self.L.fosphor_amd_colorize(self.h, int(image), palette.ctypes.data if palette is not None else None,
                                         palette.size if palette is not None else 0, 1 if defaults else 0,
                                         float(scale or 0.0), float(offset or 0.0), int(rows), out.data_ptr())
        if rv:
            raise RuntimeError("fosphor_amd_colorize -> %d" % rv)
        return out.view(torch.uint8).reshape(rows, self.n, 4)

    DETECTORS = {"peak": 0, "average": 1}	# FOSPHOR_AMD_DET_* (include/fosphor_amd_view.h)
    VIEW_OUTPUTS = ("waterfall", "histogram", "live", "max", "waterfall_rgba", "histogram_rgba")
    VIEW_FORMS = ("tiled", "tiled_lanes", "wide", "lines")

    def view(self, first_bin=0, n_cols=None, width=None, wf_src_rows=None, wf_out_rows=None, detector="peak",
             rgba=True, floats=True, wf_palette=None, histo_palette=None, wf_scale=None, wf_offset=None,
             histo_scale=None, histo_offset=None, outputs=None):
        """A zoomed, display-width view (include/fosphor_amd_view.h): the shifted columns [first_bin, first_bin + n_cols) and the
        newest wf_src_rows waterfall rows, reduced to width pixels across and wf_out_rows waterfall rows by the detector ("peak" or
        "average").  Defaults: every column from first_bin on, one pixel per column, every row, one picture row per source row.
        Returns a dict of torch device tensors: floats "waterfall" [wf_out_rows][width], "histogram" [n_bins][width], "live" and
        "max" [width] (floats=True); uint8 "waterfall_rgba" [wf_out_rows][width][4], "histogram_rgba" [n_bins][width][4] (rgba=True).
        outputs: an iterable of those names instead, to produce exactly them.  Palettes, scales and offsets as in colorize();
        None = the reference's."""
        import torch
        n_cols, wf_src_rows = self._window(first_bin, n_cols, wf_src_rows)
        if width is None:
            width = n_cols
        if wf_out_rows is None:
            wf_out_rows = wf_src_rows
        if isinstance(detector, str):
            if detector not in self.DETECTORS:
                raise ValueError("detector must be one of %s" % ", ".join(self.DETECTORS))
            detector = self.DETECTORS[detector]
        if outputs is None:
            outputs = [k for k in self.VIEW_OUTPUTS if (rgba if k.endswith("_rgba") else floats)]
        else:
            outputs = list(outputs)
            for k in outputs:
                if k not in self.VIEW_OUTPUTS:
                    raise ValueError("no such view output: %r" % (k,))
        v = _lib.View(int(first_bin), int(n_cols), int(width), int(wf_src_rows), int(wf_out_rows), int(detector))
        # shapes for the allocations only: the library checks the view itself
        w, wr = max(int(width), 1), max(int(wf_out_rows), 1)
        shapes = {"waterfall": (wr, w), "histogram": (self.n_bins, w), "live": (w,), "max": (w,),
                  "waterfall_rgba": (wr, w), "histogram_rgba": (self.n_bins, w)}
        o = _lib.ViewOut()
        res, keep = {}, []
        for k in outputs:
            t = torch.empty(shapes[k], dtype=torch.int32 if k.endswith("_rgba") else torch.float32, device="cuda")
            setattr(o, "d_" + k, t.data_ptr())
            res[k] = t
        for col, pal, scale, offset in ((o.wf_color, wf_palette, wf_scale, wf_offset),
                                        (o.histo_color, histo_palette, histo_scale, histo_offset)):
            if pal is not None:
                pal = np.ascontiguousarray(pal, dtype=np.uint32)
                keep.append(pal)
                col.palette, col.n = pal.ctypes.data, pal.size
            col.use_defaults = 1 if scale is None and offset is None else 0
            col.scale, col.offset = float(scale or 0.0), float(offset or 0.0)
        rv = self.L.fosphor_amd_view(self.h, C.byref(v), C.byref(o))
        if rv:
            _fail("fosphor_amd_view", rv, RuntimeError)
        for k in res:
            if k.endswith("_rgba"):
                res[k] = res[k].view(torch.uint8).reshape(res[k].shape + (4,))
        return res

    def view_from_render(self, render, width, wf_out_rows, **kw):
        """view() of the window that the zoom fields of a struct fosphor_render (freq_center, freq_span, wf_span) select, as the
        reference's GL side places it (fosphor_amd_view_from_render); peak detector.  Further arguments go to view()."""
        v = _lib.View()
        rv = self.L.fosphor_amd_view_from_render(self.n, self.wf_rows, C.byref(render), int(width), int(wf_out_rows), C.byref(v))
        if rv:
            _fail("fosphor_amd_view_from_render", rv, RuntimeError)
        return self.view(v.first_bin, v.n_cols, v.width, v.wf_src_rows, v.wf_out_rows, detector=v.detector, **kw)

    def view_stats(self):
        """fosphor_amd_view_stats as a dict: view launches since the instance was made, by form (VIEW_FORMS)"""
        return self._stats(self.L.fosphor_amd_view_stats, self.VIEW_FORMS)

    TRACES = {"live": 0, "maxhold": 1}		# FOSPHOR_AMD_TRACE_* (include/fosphor_amd_detect.h)
    FLOOR_MODES = {"absolute": 0, "percentile": 1}	# FOSPHOR_AMD_FLOOR_*
    DETECT_STATS = ("percentiles", "floor", "bands")
    DETECT_MAX_Q = 4
    DETECT_LANES = 1024				# FOSPHOR_AMD_DETECT_LANES
    BAND_DTYPE = np.dtype([("first", "<i4"), ("last", "<i4"), ("peak_col", "<i4"), ("peak_y", "<f4"), ("power_y", "<f4")])

    def percentiles(self, q, bins=False):
        """Per-column percentiles of the persistence histogram (fosphor_amd_percentiles): q is one value or up to 4 in ]0, 1].
        Returns the y of each percentile's bin as a float32 numpy array [n_q][N] in fft-shifted column order (NaN where a column
        is empty); bins=True: (y, bin), bin an int32 array of the same shape (-1 where a column is empty)."""
        import torch
        qa = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float32).reshape(-1)
        shape = (max(qa.size, 1), self.n)
        d_y = torch.empty(shape, dtype=torch.float32, device="cuda")
        d_bin = torch.empty(shape, dtype=torch.int32, device="cuda") if bins else None
        rv = self.L.fosphor_amd_percentiles(self.h, qa.ctypes.data, qa.size, d_y.data_ptr(), d_bin.data_ptr() if bins else None)
        if rv:
            _fail("fosphor_amd_percentiles", rv, RuntimeError)
        y = d_y.cpu().numpy()
        return (y, d_bin.cpu().numpy()) if bins else y

    def detect(self, trace="live", floor="percentile", floor_q=0.5, margin_db=6.0, threshold_y=0.0, max_gap=0, min_cols=1,
               first_bin=0, n_cols=None, max_bands=1024):
        """Occupied bands of the live or max-hold trace (fosphor_amd_detect) in the shifted columns [first_bin, first_bin + n_cols).
        floor="percentile": the threshold is the window's noise floor (the lower median over its columns of the histogram's
        floor_q percentile) plus margin_db (margin_db / 20 in y); floor="absolute": threshold_y.  Runs of up to max_gap columns
        below the threshold inside a band are closed; bands shorter than min_cols are dropped.
        Returns (result, bands): a dict with n_found, n_written, floor_bin, floor_y, threshold_y and a numpy structured array
        (BAND_DTYPE: first, last, peak_col, peak_y, power_y) of the n_written = min(n_found, max_bands) bands."""
        import torch
        if trace not in self.TRACES:
            raise ValueError("trace must be one of %s" % ", ".join(self.TRACES))
        if floor not in self.FLOOR_MODES:
            raise ValueError("floor must be one of %s" % ", ".join(self.FLOOR_MODES))
        n_cols, _ = self._window(first_bin, n_cols)
        cfg = _lib.DetectCfg(self.TRACES[trace], int(first_bin), int(n_cols), self.FLOOR_MODES[floor], float(floor_q),
                             float(margin_db) / 20.0, float(threshold_y), int(max_gap), int(min_cols))
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_res = torch.empty(C.sizeof(_lib.DetectResult), dtype=torch.uint8, device="cuda")
        d_bands = torch.empty(max(int(max_bands), 1) * self.BAND_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        rv = self.L.fosphor_amd_detect(self.h, C.byref(cfg), d_res.data_ptr(), d_bands.data_ptr(), int(max_bands))
        if rv:
            _fail("fosphor_amd_detect", rv, RuntimeError)
        res = _result(d_res, _lib.DetectResult)
        bands = d_bands.cpu().numpy().view(self.BAND_DTYPE)[:res["n_written"]].copy()
        return res, bands

    def detect_stats(self):
        """fosphor_amd_detect_stats as a dict: launches since the instance was made, by kernel (DETECT_STATS)"""
        return self._stats(self.L.fosphor_amd_detect_stats, self.DETECT_STATS)

    MASK_STATS = ("scans", "from_trace", "form_rows", "form_shared")
    MASK_MAX_EVENTS = 65536				# FOSPHOR_AMD_MASK_MAX_EVENTS (include/fosphor_amd_mask.h)
    MASK_MAX_CHANNELS = 8				# FOSPHOR_MAX_CHANNELS
    MASK_STRIP = 1024					# FOSPHOR_AMD_MASK_STRIP
    MASK_ROW_DTYPE = np.dtype([("n_over", "<i4"), ("n_under", "<i4"), ("first_col", "<i4"), ("last_col", "<i4"),
                               ("peak_col", "<i4"), ("peak_over", "<f4")])

    def mask_scan(self, upper=None, lower=None, first_bin=0, n_cols=None, rows=None, min_cols=1, channels=(), max_events=1024,
                  want_rows=True):
        """Frequency-mask trigger and channel power over the newest `rows` waterfall rows (fosphor_amd_mask_scan).  upper, lower:
        float32 device tensors [N] indexed by fft-shifted column, or None (never violated); the window is the shifted columns
        [first_bin, first_bin + n_cols).  A row triggers when at least min_cols of its columns lie over upper or under lower.
        channels: up to 8 (first, last) pairs of shifted columns, inclusive.  max_events=0: no event list.
        Returns (result, rows, events, power), numpy copies: a dict with n_triggered, n_written, newest, oldest; a structured
        array (MASK_ROW_DTYPE), one record per scanned row, j = 0 the newest (None with want_rows=False); the int32 array of the
        n_written triggered j in ascending order; the float32 array [n_channels][rows] of channel power in y."""
        import torch
        n_cols, rows = self._window(first_bin, n_cols, rows)
        channels = [(int(a), int(b)) for a, b in channels]
        if len(channels) > self.MASK_MAX_CHANNELS:
            raise ValueError("at most %d channels" % self.MASK_MAX_CHANNELS)
        for name, t in (("upper", upper), ("lower", lower)):
            if t is not None:
                _check_f32(t, self.n, name)
        cfg = _lib.MaskCfg(int(first_bin), int(n_cols), int(rows), int(min_cols), len(channels))
        for k, (a, b) in enumerate(channels):
            cfg.channels[k].first, cfg.channels[k].last = a, b
        nr = max(int(rows), 1)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_res = torch.empty(C.sizeof(_lib.MaskResult), dtype=torch.uint8, device="cuda")
        d_rows = torch.empty(nr * self.MASK_ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda") if want_rows else None
        d_ev = torch.empty(int(max_events), dtype=torch.int32, device="cuda") if max_events > 0 else None
        d_pow = torch.empty((len(channels), nr), dtype=torch.float32, device="cuda") if channels else None
        torch.cuda.synchronize()			# the limits were written on torch's stream
        rv = self.L.fosphor_amd_mask_scan(self.h, C.byref(cfg), _ptr(upper) if upper is not None else None,
                                          _ptr(lower) if lower is not None else None, d_res.data_ptr(),
                                          d_rows.data_ptr() if want_rows else None, d_ev.data_ptr() if d_ev is not None else None,
                                          int(max_events), d_pow.data_ptr() if channels else None)
        if rv:
            _fail("fosphor_amd_mask_scan", rv, RuntimeError)
        res = _result(d_res, _lib.MaskResult)
        recs = d_rows.cpu().numpy().view(self.MASK_ROW_DTYPE).copy() if want_rows else None
        events = d_ev.cpu().numpy()[:res["n_written"]].copy() if d_ev is not None else np.zeros(0, np.int32)
        power = d_pow.cpu().numpy() if channels else np.zeros((0, nr), np.float32)
        return res, recs, events, power

    def mask_from_trace(self, trace="maxhold", margin_db=6.0, spread_cols=0):
        """A limit line learnt from the live or max-hold trace (fosphor_amd_mask_from_trace): per shifted column the greatest y of
        the trace within spread_cols columns, plus margin_db (margin_db / 20 in y).  Returns a float32 device tensor [N], an
        `upper` for mask_scan."""
        import torch
        if trace not in self.TRACES:
            raise ValueError("trace must be one of %s" % ", ".join(self.TRACES))
        d_out = torch.empty(self.n, dtype=torch.float32, device="cuda")
        rv = self.L.fosphor_amd_mask_from_trace(self.h, self.TRACES[trace], float(margin_db) / 20.0, int(spread_cols), d_out.data_ptr())
        if rv:
            _fail("fosphor_amd_mask_from_trace", rv, RuntimeError)
        return d_out

    def mask_from_points(self, cols, ys):
        """A piecewise-linear limit line through the points (cols[k], ys[k]), cols strictly ascending in shifted-column units
        (fosphor_amd_mask_from_points; computed on the host).  Returns a float32 numpy array [N]."""
        c = np.ascontiguousarray(cols, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(ys, dtype=np.float32).reshape(-1)
        if c.size != y.size:
            raise ValueError("cols and ys differ in length")
        out = np.empty(self.n, np.float32)
        rv = self.L.fosphor_amd_mask_from_points(self.n, c.ctypes.data, y.ctypes.data, c.size, out.ctypes.data)
        if rv:
            _fail("fosphor_amd_mask_from_points", rv, RuntimeError)
        return out

    def mask_stats(self):
        """fosphor_amd_mask_stats as a dict: calls and launches since the instance was made, by kind and form (MASK_STATS)"""
        return self._stats(self.L.fosphor_amd_mask_stats, self.MASK_STATS)

    BURST_STATS = ("calls", "overflows", "k_count", "k_rows", "k_scan", "k_init", "k_write", "k_link", "k_reduce", "k_emit")
    BURST_MAX_RUNS = 1 << 20				# FOSPHOR_AMD_BURST_MAX_RUNS (include/fosphor_amd_burst.h)
    BURST_MAX_BURSTS = 65536				# FOSPHOR_AMD_BURST_MAX_BURSTS
    BURST_STRIP = 1024					# FOSPHOR_AMD_BURST_STRIP
    BURST_FLAGS = {"on": 1, "cut": 2, "first_col": 4, "last_col": 8}	# FOSPHOR_AMD_BURST_ON / CUT / FIRST_COL / LAST_COL
    BURST_DTYPE = np.dtype([("newest", "<i4"), ("oldest", "<i4"), ("first_col", "<i4"), ("last_col", "<i4"), ("n_cells", "<i4"),
                            ("peak_row", "<i4"), ("peak_col", "<i4"), ("peak_y", "<f4"), ("energy_y", "<f4"), ("flags", "<u4")])

    def bursts(self, threshold, first_bin=0, n_cols=None, rows=None, max_gap_cols=0, max_gap_rows=0, min_rows=1, min_cols=1,
               max_bursts=1024, max_runs=1 << 16):
        """Bursts in time and frequency over the newest `rows` waterfall rows (fosphor_amd_bursts): the connected regions of the
        cells with y > threshold, after gaps of up to max_gap_cols columns along a row are closed and runs up to max_gap_rows + 1
        rows apart that overlap in column are joined.  threshold: a float (in y, for every column), a length-N array indexed by
        fft-shifted column (uploaded), or a float32 device tensor [N] as mask_scan takes its limits.  The window is the shifted
        columns [first_bin, first_bin + n_cols).
        Returns (result, bursts): a dict with n_runs, n_components, n_found, n_written, overflow, and a numpy structured array
        (BURST_DTYPE) of the n_written records in ascending root order (newest first).  overflow = 1 (more than max_runs runs: the
        threshold sits in the noise) gives no records."""
        import torch
        n_cols, rows = self._window(first_bin, n_cols, rows, most_rows=65536)
        thr_y, d_thr = 0.0, None
        if hasattr(threshold, "data_ptr"):
            d_thr = threshold
        elif np.ndim(threshold) == 0:
            thr_y = float(threshold)
        else:
            d_thr = torch.from_numpy(np.ascontiguousarray(threshold, dtype=np.float32).reshape(-1)).cuda()
        if d_thr is not None:
            _check_f32(d_thr, self.n, "threshold", "%s must be a float, %d values, or a contiguous float32 device tensor of as many")
        cfg = _lib.BurstCfg(int(first_bin), int(n_cols), int(rows), thr_y, int(max_gap_cols), int(max_gap_rows), int(min_rows),
                            int(min_cols), int(max_runs))
        nb = max(int(max_bursts), 1)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_res = torch.empty(C.sizeof(_lib.BurstResult), dtype=torch.uint8, device="cuda")
        d_out = torch.empty(nb * self.BURST_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()			# the threshold was written on torch's stream
        rv = self.L.fosphor_amd_bursts(self.h, C.byref(cfg), d_thr.data_ptr() if d_thr is not None else None, d_res.data_ptr(),
                                       d_out.data_ptr(), int(max_bursts))
        if rv:
            _fail("fosphor_amd_bursts", rv, RuntimeError)
        res = _result(d_res, _lib.BurstResult)
        recs = d_out.cpu().numpy().view(self.BURST_DTYPE)[:res["n_written"]].copy()
        return res, recs

    def burst_stats(self):
        """fosphor_amd_burst_stats as a dict: calls, overflows and launches by kernel since the instance was made (BURST_STATS)"""
        return self._stats(self.L.fosphor_amd_burst_stats, self.BURST_STATS)

    EXTRACT_STATS = ("calls", "k_tile", "k_wave", "jobs_tile", "jobs_wave", "samples")
    EXTRACT_MAX_JOBS = 4096				# FOSPHOR_AMD_EXTRACT_MAX_JOBS (include/fosphor_amd_extract.h)
    EXTRACT_MAX_DECIM = 1024				# FOSPHOR_AMD_EXTRACT_MAX_DECIM
    EXTRACT_MAX_TAPS = 8192				# FOSPHOR_AMD_EXTRACT_MAX_TAPS
    EXTRACT_TILE_OUT = 256				# FOSPHOR_AMD_EXTRACT_TILE_OUT
    EXTRACT_TILE_LDS = 6656				# FOSPHOR_AMD_EXTRACT_TILE_LDS
    EXTRACT_WAVE_OUT = 4				# FOSPHOR_AMD_EXTRACT_WAVE_OUT
    EXTRACT_DTYPE = np.dtype([("first", "<i8"), ("out_offset", "<i8"), ("n_out", "<i4"), ("decim", "<i4"), ("phase_inc", "<u4"),
                              ("phase0", "<u4"), ("taps_offset", "<i4"), ("n_taps", "<i4")])

    @staticmethod
    def extract_form(decim, n_taps):
        """the kernel form of a job, "tile" or "wave": a function of (D, T) alone (include/fosphor_amd_extract.h)"""
        row = (Fosphor.EXTRACT_TILE_OUT + (int(n_taps) - 1) // int(decim) + 1) | 1
        return "tile" if int(decim) * row <= Fosphor.EXTRACT_TILE_LDS else "wave"

    @staticmethod
    def extract_design(decim, n_taps, guard=0.8):
        """fosphor_amd_extract_design: the Hamming-windowed sinc low-pass of n_taps float32 taps for decimation decim, cutoff
        guard / (2 * decim) cycles per sample; the taps sum to 1 and are symmetric"""
        out = np.empty(max(int(n_taps), 1), np.float32)
        rv = _lib.load().fosphor_amd_extract_design(int(decim), int(n_taps), float(guard), out.ctypes.data)
        if rv:
            _fail("fosphor_amd_extract_design", rv, ValueError)
        return out

    def extract_from_burst(self, burst, newest_first_sample, row_hop, max_decim=64, guard=0.8):
        """fosphor_amd_extract_from_burst: (job, n_taps) for one record of bursts().  newest_first_sample: the index in the
        caller's stream of the first sample of the spectrum in ring row 0; row_hop: samples between consecutive rows' spectra.
        job is a one-element EXTRACT_DTYPE array with out_offset = taps_offset = 0: the caller places it."""
        b = _lib.Burst.from_buffer_copy(np.asarray(burst, self.BURST_DTYPE).reshape(1).tobytes())
        job, taps = _lib.ExtractJob(), C.c_int(0)
        rv = self.L.fosphor_amd_extract_from_burst(C.byref(b), self.n, int(newest_first_sample), int(row_hop), int(max_decim),
                                                   float(guard), C.byref(job), C.byref(taps))
        if rv:
            _fail("fosphor_amd_extract_from_burst", rv, ValueError)
        return np.frombuffer(bytes(job), self.EXTRACT_DTYPE).copy(), taps.value

    def extract(self, d_iq, jobs, taps, iq_format=None, n_samples=None):
        """Baseband IQ of up to 4096 jobs in one call (fosphor_amd_extract): mix, real FIR, decimate, over samples that are
        already in device memory.  d_iq: a contiguous device tensor of the stream (complex64 / float32 pairs for fp32, int16 or
        float16 pairs for sc16 / fp16) or a raw device pointer with n_samples; jobs: an EXTRACT_DTYPE array (out_offset is
        honoured; ranges must not overlap); taps: float32 values (uploaded) or a float32 device tensor, addressed by the jobs'
        taps_offset / n_taps; iq_format: "fp32" / "fp16" / "sc16", a FOSPHOR_AMD_IQ_* number, or None for the instance's.
        Returns a list with one torch complex64 view per job, into one device buffer."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.EXTRACT_DTYPE)
        fmt = -1 if iq_format is None else IQ_FORMATS[iq_format] if isinstance(iq_format, str) else int(iq_format)
        n_samples = _iq_count(d_iq, n_samples, "d_iq", floats=False)
        if hasattr(taps, "data_ptr"):
            d_taps = taps
            if d_taps.dtype != torch.float32 or not d_taps.is_cuda or not d_taps.is_contiguous():
                raise ValueError("taps must be float32 values or a contiguous float32 device tensor")
        else:
            d_taps = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)).cuda()
        cap = int((jobs["out_offset"] + jobs["n_out"]).max()) if jobs.size else 0
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 1), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()			# the taps (and the caller's samples) were written on torch's stream
        rv = self.L.fosphor_amd_extract(self.h, _ptr(d_iq), int(n_samples), fmt, jobs.ctypes.data, int(jobs.size),
                                        d_taps.data_ptr(), int(d_taps.numel()), d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_extract", rv, RuntimeError)
        return [d_out[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] for j in jobs]

    def extract_stats(self):
        """fosphor_amd_extract_stats as a dict: calls, launches and jobs by kernel form, input samples spanned (EXTRACT_STATS)"""
        return self._stats(self.L.fosphor_amd_extract_stats, self.EXTRACT_STATS)

    MEASURE_STATS = ("calls", "k_wave", "k_split", "k_combine", "jobs_wave", "jobs_split", "samples")
    MEASURE_MAX_JOBS = 4096				# FOSPHOR_AMD_MEASURE_MAX_JOBS (include/fosphor_amd_measure.h)
    MEASURE_WAVE_MAX = 4096				# FOSPHOR_AMD_MEASURE_WAVE_MAX
    MEASURE_CHUNK = 8192				# FOSPHOR_AMD_MEASURE_CHUNK
    MEASURE_FORMS = ("wave", "split")			# FOSPHOR_AMD_MEASURE_FORM_*
    MEASURE_JOB_DTYPE = np.dtype([("offset", "<i8"), ("n", "<i4"), ("threshold", "<f4")])
    MEASURE_RECORD_DTYPE = np.dtype([("n_above", "<i4"), ("first_above", "<i4"), ("last_above", "<i4"), ("n_edges", "<i4"),
                                     ("peak_index", "<i4"), ("peak_power", "<f4"), ("s_re", "<f8"), ("s_im", "<f8"),
                                     ("s_p", "<f8"), ("s_p2", "<f8"), ("s_zz_re", "<f8"), ("s_zz_im", "<f8"), ("r1_re", "<f8"),
                                     ("r1_im", "<f8"), ("n", "<i4"), ("form", "<i4")])
    MEASURE_VALUES = tuple(k for k, _ in _lib.MeasureValues._fields_)

    @staticmethod
    def measure_form(n):
        """the kernel form of a job, "wave" or "split": a function of n alone (include/fosphor_amd_measure.h)"""
        return "wave" if int(n) <= Fosphor.MEASURE_WAVE_MAX else "split"

    @staticmethod
    def measure_jobs(jobs, threshold=None):
        """a MEASURE_JOB_DTYPE array from one, or from an EXTRACT_DTYPE array and threshold= (fosphor_amd_measure_from_extract:
        each job measures what the extract job wrote, offset = out_offset, n = n_out)"""
        jobs = np.atleast_1d(np.asarray(jobs))
        if jobs.dtype != Fosphor.EXTRACT_DTYPE:
            if threshold is not None:
                raise ValueError("threshold= goes with extract jobs; measure jobs carry their own")
            return np.ascontiguousarray(jobs, dtype=Fosphor.MEASURE_JOB_DTYPE)
        if threshold is None:
            raise ValueError("extract jobs need threshold=")
        L = _lib.load()
        out = np.zeros(jobs.size, Fosphor.MEASURE_JOB_DTYPE)
        for i, e in enumerate(np.ascontiguousarray(jobs)):
            job = _lib.MeasureJob()
            rv = L.fosphor_amd_measure_from_extract(e.tobytes(), float(threshold), C.byref(job))
            if rv:
                _fail("fosphor_amd_measure_from_extract", rv, ValueError)
            out[i] = (job.offset, job.n, job.threshold)
        return out

    def measure(self, d_iq, jobs, n_samples=None, threshold=None):
        """One record per job, up to 4096 jobs in one call (fosphor_amd_measure): samples above a threshold, edges, peak, and the
        double-precision sums of y, p, p^2, y^2 and y[m + 1] conj(y[m]) over float32 IQ that is already in device memory.  d_iq: a
        contiguous device tensor (complex64 or float32 pairs; what extract() wrote) or a raw device pointer with n_samples;
        jobs: a MEASURE_JOB_DTYPE array, or an EXTRACT_DTYPE array with threshold= (measure_jobs).  Returns a
        MEASURE_RECORD_DTYPE array copied from the device, in job order."""
        import torch
        jobs = self.measure_jobs(jobs, threshold)
        n_samples = _iq_count(d_iq, n_samples, "d_iq")
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_rec = torch.empty(max(jobs.size, 1) * self.MEASURE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()			# the caller's samples were written on torch's stream
        rv = self.L.fosphor_amd_measure(self.h, _ptr(d_iq), int(n_samples), jobs.ctypes.data, int(jobs.size), d_rec.data_ptr())
        if rv:
            _fail("fosphor_amd_measure", rv, RuntimeError)
        return d_rec.cpu().numpy().view(self.MEASURE_RECORD_DTYPE)[:jobs.size].copy()

    @staticmethod
    def measure_host(iq, jobs):
        """fosphor_amd_measure_host: the same records on the host, no GPU.  iq: complex64 or float32 pairs"""
        iq = _float_pairs(iq)
        jobs = Fosphor.measure_jobs(jobs)
        out = np.zeros(max(jobs.size, 1), Fosphor.MEASURE_RECORD_DTYPE)
        keep = _or_dummy(iq)
        rv = _lib.load().fosphor_amd_measure_host(keep.ctypes.data, iq.size // 2, jobs.ctypes.data, int(jobs.size), out.ctypes.data)
        if rv:
            _fail("fosphor_amd_measure_host", rv, ValueError)
        return out[:jobs.size]

    @staticmethod
    def measure_derive(records, sample_rate):
        """fosphor_amd_measure_derive per record: a list of dicts of MEASURE_VALUES (dB, Hz, ratios, seconds; pulses an int)"""
        L = _lib.load()
        out = []
        for r in np.ascontiguousarray(np.atleast_1d(records), dtype=Fosphor.MEASURE_RECORD_DTYPE):
            v = _lib.MeasureValues()
            rv = L.fosphor_amd_measure_derive(r.tobytes(), float(sample_rate), C.byref(v))
            if rv:
                _fail("fosphor_amd_measure_derive", rv, ValueError)
            d = {k: getattr(v, k) for k in Fosphor.MEASURE_VALUES}
            d["pulses"] = int(d["pulses"])
            out.append(d)
        return out

    def measure_stats(self):
        """fosphor_amd_measure_stats as a dict: calls, launches by kernel, jobs by form, samples (MEASURE_STATS)"""
        return self._stats(self.L.fosphor_amd_measure_stats, self.MEASURE_STATS)

    DEMOD_STATS = ("calls", "k_direct", "k_avg", "jobs_direct", "jobs_avg", "samples", "outputs")
    DEMOD_MAX_JOBS = 4096				# FOSPHOR_AMD_DEMOD_MAX_JOBS (include/fosphor_amd_demod.h)
    DEMOD_MAX_AVG = 256					# FOSPHOR_AMD_DEMOD_MAX_AVG
    DEMOD_TILE = 2048					# FOSPHOR_AMD_DEMOD_TILE
    DEMOD_MODES = {"power": 0, "phase": 1, "fm": 2}	# FOSPHOR_AMD_DEMOD_*
    DEMOD_JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("mode", "<i4"), ("avg", "<i4"),
                                ("reserved", "<i4")])

    @staticmethod
    def _demod_mode(mode):
        if isinstance(mode, str):
            if mode not in Fosphor.DEMOD_MODES:
                raise ValueError("mode must be one of %s" % ", ".join(Fosphor.DEMOD_MODES))
            return Fosphor.DEMOD_MODES[mode]
        return int(mode)

    @staticmethod
    def demod_n_out(mode, n, avg=1):
        """fosphor_amd_demod_n_out: the outputs of a job of n samples, n_trace // avg (n_trace = n, or n - 1 for "fm")"""
        rv = _lib.load().fosphor_amd_demod_n_out(Fosphor._demod_mode(mode), int(n), int(avg))
        if rv < 0:
            _fail("fosphor_amd_demod_n_out", rv, ValueError)
        return rv

    @staticmethod
    def demod_jobs(extract_jobs, mode="fm", avg=1):
        """a DEMOD_JOB_DTYPE array from an EXTRACT_DTYPE array (fosphor_amd_demod_from_extract: each job demodulates what the
        extract job wrote, offset = out_offset, n = n_out), the outputs placed back to back from out_offset 0 on"""
        L = _lib.load()
        ejobs = np.ascontiguousarray(np.atleast_1d(extract_jobs), dtype=Fosphor.EXTRACT_DTYPE)
        out = np.zeros(ejobs.size, Fosphor.DEMOD_JOB_DTYPE)
        at = 0
        for i, e in enumerate(ejobs):
            job = _lib.DemodJob()
            rv = L.fosphor_amd_demod_from_extract(e.tobytes(), Fosphor._demod_mode(mode), int(avg), C.byref(job))
            if rv:
                _fail("fosphor_amd_demod_from_extract", rv, ValueError)
            out[i] = (job.offset, at, job.n, job.mode, job.avg, job.reserved)
            at += Fosphor.demod_n_out(job.mode, job.n, job.avg)
        return out

    @staticmethod
    def _demod_outs(jobs):
        return _outs(jobs, lambda j: Fosphor.demod_n_out(int(j["mode"]), int(j["n"]), int(j["avg"])))

    def demod(self, d_iq, jobs, n_samples=None):
        """One float32 trace per job, up to 4096 jobs in one call (fosphor_amd_demod): power, phase in turns or the phase step
        between consecutive samples in turns ("fm"), integrated and dumped over avg trace values, over float32 IQ that is already
        in device memory.  d_iq: a contiguous device tensor (complex64 or float32 pairs; what extract() wrote) or a raw device
        pointer with n_samples; jobs: a DEMOD_JOB_DTYPE array (out_offset is honoured; ranges must not overlap; demod_jobs()
        makes one from extract jobs).  Returns a list with one torch float32 view per job, into one device buffer."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.DEMOD_JOB_DTYPE)
        n_samples = _iq_count(d_iq, n_samples, "d_iq")
        n_out, cap = self._demod_outs(jobs)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 1), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()			# the caller's samples were written on torch's stream
        rv = self.L.fosphor_amd_demod(self.h, _ptr(d_iq), int(n_samples), jobs.ctypes.data, int(jobs.size), d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_demod", rv, RuntimeError)
        return [d_out[int(j["out_offset"]):int(j["out_offset"]) + n] for j, n in zip(jobs, n_out)]

    @staticmethod
    def demod_host(iq, jobs):
        """fosphor_amd_demod_host: the same traces on the host, no GPU.  iq: complex64 or float32 pairs.  Returns a list with one
        float32 array per job, views of one buffer"""
        iq = _float_pairs(iq)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.DEMOD_JOB_DTYPE)
        n_out, cap = Fosphor._demod_outs(jobs)
        out = np.zeros(max(cap, 1), np.float32)
        keep = _or_dummy(iq)
        rv = _lib.load().fosphor_amd_demod_host(keep.ctypes.data, iq.size // 2, jobs.ctypes.data, int(jobs.size), out.ctypes.data, cap)
        if rv:
            _fail("fosphor_amd_demod_host", rv, ValueError)
        return [out[int(j["out_offset"]):int(j["out_offset"]) + n] for j, n in zip(jobs, n_out)]

    @staticmethod
    def atan2_turns(y, x):
        """fosphor_amd_atan2_turns as the library compiled it: the angle of (x, y) in turns, float32, element-wise over float64"""
        y, x = np.broadcast_arrays(np.asarray(y, np.float64), np.asarray(x, np.float64))
        shape = y.shape
        y, x = np.ascontiguousarray(y).reshape(-1), np.ascontiguousarray(x).reshape(-1)
        out = np.zeros(max(y.size, 1), np.float32)
        rv = _lib.load().fosphor_amd_demod_atan2_turns_n(y.ctypes.data, x.ctypes.data, int(y.size), out.ctypes.data)
        if rv:
            raise ValueError("fosphor_amd_demod_atan2_turns_n -> %d" % rv)
        return out[:y.size].reshape(shape)

    def demod_stats(self):
        """fosphor_amd_demod_stats as a dict: calls, launches by kernel, jobs by form, samples, outputs (DEMOD_STATS)"""
        return self._stats(self.L.fosphor_amd_demod_stats, self.DEMOD_STATS)

    CORRELATE_STATS = ("calls", "k_tile", "k_combine", "jobs", "lags", "macs")
    CORRELATE_MAX_JOBS = 4096				# FOSPHOR_AMD_CORRELATE_MAX_JOBS (include/fosphor_amd_correlate.h)
    CORRELATE_MAX_TPL = 1024				# FOSPHOR_AMD_CORRELATE_MAX_TPL
    CORRELATE_TILE = 1024				# FOSPHOR_AMD_CORRELATE_TILE
    CORRELATE_TRACES = {"none": 0, "rho": 1, "c": 2}	# FOSPHOR_AMD_CORRELATE_TRACE_*
    CORRELATE_JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("tpl_offset", "<i8"), ("n", "<i4"),
                                    ("tpl_len", "<i4"), ("trace", "<i4"), ("threshold", "<f4")])
    CORRELATE_RECORD_DTYPE = np.dtype([("n_lags", "<i4"), ("n_above", "<i4"), ("first_above", "<i4"), ("last_above", "<i4"),
                                       ("n_edges", "<i4"), ("peak_lag", "<i4"), ("peak_rho", "<f4"), ("tpl_len", "<i4"),
                                       ("peak_c_re", "<f8"), ("peak_c_im", "<f8"), ("peak_energy", "<f8"), ("tpl_energy", "<f8")])
    CORRELATE_VALUES = tuple(k for k, _ in _lib.CorrelateValues._fields_)

    @staticmethod
    def _correlate_trace(trace):
        if isinstance(trace, str):
            if trace not in Fosphor.CORRELATE_TRACES:
                raise ValueError("trace must be one of %s" % ", ".join(Fosphor.CORRELATE_TRACES))
            return Fosphor.CORRELATE_TRACES[trace]
        return int(trace)

    @staticmethod
    def correlate_n_out(trace, n, tpl_len):
        """fosphor_amd_correlate_n_out: the trace floats of a job of n samples: 0, n_lags or 2 * n_lags, n_lags = max(n - T + 1, 0)"""
        rv = _lib.load().fosphor_amd_correlate_n_out(Fosphor._correlate_trace(trace), int(n), int(tpl_len))
        if rv < 0:
            _fail("fosphor_amd_correlate_n_out", rv, ValueError)
        return rv

    @staticmethod
    def correlate_jobs(extract_jobs, tpl_offset, tpl_len, trace="none", threshold=np.inf):
        """a CORRELATE_JOB_DTYPE array from an EXTRACT_DTYPE array (fosphor_amd_correlate_from_extract: each job correlates what
        the extract job wrote, offset = out_offset, n = n_out, against the template at tpl_offset), the traces placed back to back
        from out_offset 0 on (a "c" trace has an even number of floats, so each begins on an even one)"""
        L = _lib.load()
        ejobs = np.ascontiguousarray(np.atleast_1d(extract_jobs), dtype=Fosphor.EXTRACT_DTYPE)
        out = np.zeros(ejobs.size, Fosphor.CORRELATE_JOB_DTYPE)
        code = Fosphor._correlate_trace(trace)
        at = 0
        for i, e in enumerate(ejobs):
            job = _lib.CorrelateJob()
            rv = L.fosphor_amd_correlate_from_extract(e.tobytes(), int(tpl_offset), int(tpl_len), code, float(threshold), C.byref(job))
            if rv:
                _fail("fosphor_amd_correlate_from_extract", rv, ValueError)
            out[i] = (job.offset, at if code else 0, job.tpl_offset, job.n, job.tpl_len, job.trace, job.threshold)
            at += Fosphor.correlate_n_out(code, job.n, job.tpl_len)
        return out

    @staticmethod
    def _correlate_outs(jobs):
        return _outs(jobs, lambda j: Fosphor.correlate_n_out(int(j["trace"]), int(j["n"]), int(j["tpl_len"])))

    @staticmethod
    def _correlate_views(buf, jobs, n_out, complex_view):
        views = []
        for j, n in zip(jobs, n_out):
            at, trace = int(j["out_offset"]), int(j["trace"])
            if trace == 0:
                views.append(None)
            elif trace == 1:
                views.append(buf[at:at + n])
            else:
                views.append(complex_view(buf[at:at + n]))
        return views

    def correlate(self, d_iq, jobs, tpl, n_samples=None, n_tpl=None):
        """One record per job and, where the job asks for one, its trace, up to 4096 jobs in one call (fosphor_amd_correlate):
        the sliding correlation of float32 IQ that is already in device memory against templates of up to 1024 samples, "valid"
        lags only; rho = |c|^2 / (E Et) per lag, the peak, the lags above the job's threshold.  d_iq: a contiguous device tensor
        (complex64 or float32 pairs; what extract() wrote) or a raw device pointer with n_samples; jobs: a CORRELATE_JOB_DTYPE
        array (correlate_jobs() makes one from extract jobs); tpl: a numpy array of complex64 or float32 pairs (uploaded), such a
        device tensor -- d_iq itself to correlate one burst against another -- or a raw device pointer with n_tpl.
        Returns (records, views): a CORRELATE_RECORD_DTYPE array copied from the device, in job order, and a list with, per job,
        a torch float32 view ("rho"), a complex64 view ("c") or None, into one device buffer.  A complex64 view begins on an
        even float: a "c" job with an odd out_offset, which the C entry point takes, is a ValueError here."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.CORRELATE_JOB_DTYPE)
        if np.any((jobs["trace"] == 2) & (jobs["out_offset"] & 1 != 0)):
            raise ValueError("a \"c\" trace needs an even out_offset")
        if isinstance(tpl, np.ndarray):
            tpl = torch.from_numpy(_or_dummy(_float_pairs(tpl))).cuda()
        n_samples = _iq_count(d_iq, n_samples, "samples")
        n_tpl = _iq_count(tpl, n_tpl, "tpl")
        n_out, cap = self._correlate_outs(jobs)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 1), dtype=torch.float32, device="cuda")
        d_rec = torch.empty(max(jobs.size, 1) * self.CORRELATE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()			# the caller's samples were written on torch's stream
        rv = self.L.fosphor_amd_correlate(self.h, _ptr(d_iq), n_samples, _ptr(tpl), n_tpl, jobs.ctypes.data, int(jobs.size),
                                          d_rec.data_ptr(), d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_correlate", rv, RuntimeError)
        records = d_rec.cpu().numpy().view(self.CORRELATE_RECORD_DTYPE)[:jobs.size].copy()
        return records, self._correlate_views(d_out, jobs, n_out, lambda v: v.view(torch.complex64))

    @staticmethod
    def correlate_host(iq, jobs, tpl):
        """fosphor_amd_correlate_host: the same records and traces on the host, no GPU.  iq, tpl: complex64 or float32 pairs.
        Returns (records, views), the views float32 ("rho") or complex64 ("c") arrays into one buffer, or None"""
        iq, tpl = _float_pairs(iq), _float_pairs(tpl)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.CORRELATE_JOB_DTYPE)
        n_out, cap = Fosphor._correlate_outs(jobs)
        out = np.zeros(max(cap, 2), np.float32)
        records = np.zeros(max(jobs.size, 1), Fosphor.CORRELATE_RECORD_DTYPE)
        keep = _or_dummy(iq), _or_dummy(tpl)
        rv = _lib.load().fosphor_amd_correlate_host(keep[0].ctypes.data, iq.size // 2, keep[1].ctypes.data, tpl.size // 2,
                                                    jobs.ctypes.data, int(jobs.size), records.ctypes.data, out.ctypes.data, cap)
        if rv:
            _fail("fosphor_amd_correlate_host", rv, ValueError)
        return records[:jobs.size], Fosphor._correlate_views(out, jobs, n_out, lambda v: v.view(np.complex64))

    @staticmethod
    def correlate_derive(records, sample_rate):
        """fosphor_amd_correlate_derive per record: a list of dicts of CORRELATE_VALUES (seconds, ratios, dB, turns; detections
        an int)"""
        L = _lib.load()
        out = []
        for r in np.ascontiguousarray(np.atleast_1d(records), dtype=Fosphor.CORRELATE_RECORD_DTYPE):
            v = _lib.CorrelateValues()
            rv = L.fosphor_amd_correlate_derive(r.tobytes(), float(sample_rate), C.byref(v))
            if rv:
                _fail("fosphor_amd_correlate_derive", rv, ValueError)
            d = {k: getattr(v, k) for k in Fosphor.CORRELATE_VALUES}
            d["detections"] = int(d["detections"])
            out.append(d)
        return out

    def correlate_stats(self):
        """fosphor_amd_correlate_stats as a dict: calls, launches by kernel, jobs, lags, complex multiply-adds (CORRELATE_STATS)"""
        return self._stats(self.L.fosphor_amd_correlate_stats, self.CORRELATE_STATS)

    PSD_STATS = ("calls", "k_group", "k_wave", "k_combine", "jobs", "segments")
    PSD_MAX_JOBS = 4096					# FOSPHOR_AMD_PSD_MAX_JOBS (include/fosphor_amd_psd.h)
    PSD_MIN_LOG, PSD_MAX_LOG = 6, 10			# FOSPHOR_AMD_PSD_MIN_LOG, FOSPHOR_AMD_PSD_MAX_LOG
    PSD_TILE = 32					# FOSPHOR_AMD_PSD_TILE
    PSD_PRES = {"none": 0, "square": 1, "fourth": 2, "magsq": 3}	# FOSPHOR_AMD_PSD_PRE_*
    PSD_TRACES = {"none": 0, "power": 1}		# FOSPHOR_AMD_PSD_TRACE_*
    PSD_WINDOWS = {"rect": 0, "hann": 1, "blackman_harris": 2}	# FOSPHOR_AMD_PSD_WINDOW_*
    PSD_LDS = {"group": 37904, "wave": 19008, "combine": 22528}	# FOSPHOR_AMD_PSD_LDS_*
    PSD_JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("win_offset", "<i8"), ("n", "<i4"), ("fft_len_log", "<i4"),
                              ("hop", "<i4"), ("pre", "<i4"), ("trace", "<i4"), ("obw_fraction", "<f4"), ("xdb_ratio", "<f4"),
                              ("reserved", "<i4")])
    PSD_RECORD_DTYPE = np.dtype([("n_seg", "<i4"), ("fft_len", "<i4"), ("peak_bin", "<i4"), ("peak_power", "<f4"), ("obw_lo", "<i4"),
                                 ("obw_hi", "<i4"), ("xdb_lo", "<i4"), ("xdb_hi", "<i4"), ("total", "<f8"), ("m1", "<f8"),
                                 ("m2", "<f8"), ("win_energy", "<f8")])
    PSD_VALUES = tuple(k for k, _ in _lib.PsdValues._fields_)

    @staticmethod
    def _psd_code(table, what, v):
        if isinstance(v, str):
            if v not in table:
                raise ValueError("%s must be one of %s" % (what, ", ".join(table)))
            return table[v]
        return int(v)

    @staticmethod
    def psd_n_seg(n, fft_len_log, hop):
        """fosphor_amd_psd_n_seg: the segments of a job of n samples, n < L ? 0 : (n - L) // hop + 1"""
        rv = _lib.load().fosphor_amd_psd_n_seg(int(n), int(fft_len_log), int(hop))
        if rv < 0:
            _fail("fosphor_amd_psd_n_seg", rv, ValueError)
        return rv

    @staticmethod
    def psd_window(kind, fft_len_log):
        """fosphor_amd_psd_window: "rect", "hann" or "blackman_harris" in periodic form, float32 [2^fft_len_log]"""
        if not Fosphor.PSD_MIN_LOG <= int(fft_len_log) <= Fosphor.PSD_MAX_LOG:
            raise ValueError("fft_len_log must be %d .. %d" % (Fosphor.PSD_MIN_LOG, Fosphor.PSD_MAX_LOG))
        out = np.zeros(1 << int(fft_len_log), np.float32)
        rv = _lib.load().fosphor_amd_psd_window(Fosphor._psd_code(Fosphor.PSD_WINDOWS, "kind", kind), int(fft_len_log), out.ctypes.data)
        if rv:
            _fail("fosphor_amd_psd_window", rv, ValueError)
        return out

    @staticmethod
    def psd_twiddles():
        """fosphor_amd_psd_twiddles: the table of the pass, e^(-2 pi i m / 1024) for m < 512, complex128 [512]"""
        out = np.zeros(512, np.complex128)
        rv = _lib.load().fosphor_amd_psd_twiddles(out.ctypes.data)
        if rv:
            _fail("fosphor_amd_psd_twiddles", rv, ValueError)
        return out

    @staticmethod
    def psd_ratio_from_db(db):
        """fosphor_amd_psd_ratio_from_db: 10^(db / 10) for db <= 0: what a job's xdb_ratio wants"""
        return _lib.load().fosphor_amd_psd_ratio_from_db(float(db))

    @staticmethod
    def psd_jobs(extract_jobs, fft_len_log, hop=None, win_offset=0, pre="none", trace="none", obw_fraction=0.99, xdb=-26.0):
        """a PSD_JOB_DTYPE array from an EXTRACT_DTYPE array (fosphor_amd_psd_from_extract: each job takes the spectrum of what the
        extract job wrote, offset = out_offset, n = n_out), the traces placed back to back from out_offset 0 on.  hop: L // 2 by
        default; xdb: dB below the peak, at most 0"""
        L = _lib.load()
        ejobs = np.ascontiguousarray(np.atleast_1d(extract_jobs), dtype=Fosphor.EXTRACT_DTYPE)
        out = np.zeros(ejobs.size, Fosphor.PSD_JOB_DTYPE)
        pre, trace = Fosphor._psd_code(Fosphor.PSD_PRES, "pre", pre), Fosphor._psd_code(Fosphor.PSD_TRACES, "trace", trace)
        hop = (1 << int(fft_len_log)) // 2 if hop is None else int(hop)
        ratio = Fosphor.psd_ratio_from_db(xdb)
        at = 0
        for i, e in enumerate(ejobs):
            job = _lib.PsdJob()
            rv = L.fosphor_amd_psd_from_extract(e.tobytes(), int(win_offset), int(fft_len_log), hop, pre, trace, float(obw_fraction),
                                                ratio, C.byref(job))
            if rv:
                _fail("fosphor_amd_psd_from_extract", rv, ValueError)
            out[i] = (job.offset, at if trace else 0, job.win_offset, job.n, job.fft_len_log, job.hop, job.pre, job.trace,
                      job.obw_fraction, job.xdb_ratio, 0)
            at += Fosphor._psd_n_out(out[i])
        return out

    @staticmethod
    def _psd_n_out(j):
        """the trace floats of a job: L with a trace and a segment, else 0"""
        return (1 << int(j["fft_len_log"])) if int(j["trace"]) and Fosphor.psd_n_seg(j["n"], j["fft_len_log"], j["hop"]) > 0 else 0

    @staticmethod
    def _psd_views(buf, jobs, n_out):
        return [buf[int(j["out_offset"]):int(j["out_offset"]) + n] if n else None for j, n in zip(jobs, n_out)]

    def psd(self, d_iq, jobs, win, n_samples=None, n_win=None):
        """One record per job and, where the job asks for one, its trace, up to 4096 jobs in one call (fosphor_amd_psd): Welch's
        averaged power spectrum of float32 IQ that is already in device memory, segments of L = 64 .. 1024 samples, hop apart,
        windowed, transformed in double; peak, occupied bandwidth, x-dB bandwidth and moments in the record.  d_iq: a contiguous
        device tensor (complex64 or float32 pairs; what extract() wrote) or a raw device pointer with n_samples; jobs: a
        PSD_JOB_DTYPE array (psd_jobs() makes one from extract jobs); win: a float32 numpy array (uploaded; psd_window() makes
        one), such a device tensor, or a raw device pointer with n_win.
        Returns (records, views): a PSD_RECORD_DTYPE array copied from the device, in job order, and a list with, per job, a
        torch float32 view of L values in ascending frequency, DC at L // 2, or None, into one device buffer."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.PSD_JOB_DTYPE)
        if isinstance(win, np.ndarray):
            win = torch.from_numpy(np.ascontiguousarray(win if win.size else np.zeros(1), dtype=np.float32).reshape(-1)).cuda()
        n_samples = _iq_count(d_iq, n_samples, "samples")
        if n_win is None:
            if not hasattr(win, "numel"):
                raise ValueError("a raw device pointer needs n_win")
            if not win.is_contiguous() or str(win.dtype) != "torch.float32":
                raise ValueError("win must be a contiguous float32 tensor")
            n_win = win.numel()
        n_out, cap = _outs(jobs, self._psd_n_out)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 1), dtype=torch.float32, device="cuda")
        d_rec = torch.empty(max(jobs.size, 1) * self.PSD_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()			# the caller's samples were written on torch's stream
        rv = self.L.fosphor_amd_psd(self.h, _ptr(d_iq), n_samples, _ptr(win), int(n_win), jobs.ctypes.data, int(jobs.size),
                                    d_rec.data_ptr(), d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_psd", rv, RuntimeError)
        records = d_rec.cpu().numpy().view(self.PSD_RECORD_DTYPE)[:jobs.size].copy()
        return records, self._psd_views(d_out, jobs, n_out)

    @staticmethod
    def psd_host(iq, jobs, win):
        """fosphor_amd_psd_host: the same records and traces on the host, no GPU.  iq: complex64 or float32 pairs; win: float32.
        Returns (records, views), the views float32 arrays into one buffer, or None"""
        iq = _float_pairs(iq)
        win = np.ascontiguousarray(win, dtype=np.float32).reshape(-1)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.PSD_JOB_DTYPE)
        n_out, cap = _outs(jobs, Fosphor._psd_n_out)
        out = np.zeros(max(cap, 1), np.float32)
        records = np.zeros(max(jobs.size, 1), Fosphor.PSD_RECORD_DTYPE)
        keep = _or_dummy(iq), _or_dummy(win)
        rv = _lib.load().fosphor_amd_psd_host(keep[0].ctypes.data, iq.size // 2, keep[1].ctypes.data, win.size, jobs.ctypes.data,
                                              int(jobs.size), records.ctypes.data, out.ctypes.data, cap)
        if rv:
            _fail("fosphor_amd_psd_host", rv, ValueError)
        return records[:jobs.size], Fosphor._psd_views(out, jobs, n_out)

    @staticmethod
    def psd_derive(records, sample_rate):
        """fosphor_amd_psd_derive per record: a list of dicts of PSD_VALUES (Hz relative to the burst's centre, dB, power)"""
        L = _lib.load()
        out = []
        for r in np.ascontiguousarray(np.atleast_1d(records), dtype=Fosphor.PSD_RECORD_DTYPE):
            v = _lib.PsdValues()
            rv = L.fosphor_amd_psd_derive(r.tobytes(), float(sample_rate), C.byref(v))
            if rv:
                _fail("fosphor_amd_psd_derive", rv, ValueError)
            out.append({k: getattr(v, k) for k in Fosphor.PSD_VALUES})
        return out

    def psd_stats(self):
        """fosphor_amd_psd_stats as a dict: calls, launches by kernel, jobs, segments (PSD_STATS)"""
        return self._stats(self.L.fosphor_amd_psd_stats, self.PSD_STATS)

    RESAMPLE_STATS = ("calls", "k_tile", "k_direct", "jobs_tile", "jobs_direct", "outputs", "macs")
    RESAMPLE_MAX_JOBS = 4096				# FOSPHOR_AMD_RESAMPLE_MAX_JOBS (include/fosphor_amd_resample.h)
    RESAMPLE_MAX_UP = 256				# FOSPHOR_AMD_RESAMPLE_MAX_UP
    RESAMPLE_MAX_DOWN = 256				# FOSPHOR_AMD_RESAMPLE_MAX_DOWN
    RESAMPLE_MAX_BRANCH = 64				# FOSPHOR_AMD_RESAMPLE_MAX_BRANCH
    RESAMPLE_TILE = 512					# FOSPHOR_AMD_RESAMPLE_TILE
    RESAMPLE_TILE_LDS = 40960				# FOSPHOR_AMD_RESAMPLE_TILE_LDS
    RESAMPLE_DIRECT_OUT = 256				# FOSPHOR_AMD_RESAMPLE_DIRECT_OUT
    RESAMPLE_JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("phase0", "<i8"), ("n", "<i4"), ("n_out", "<i4"),
                                   ("up", "<i4"), ("down", "<i4"), ("taps_offset", "<i4"), ("n_taps", "<i4")])

    @staticmethod
    def resample_form(up, down, n_taps):
        """the kernel form of a job, "tile" or "direct": a function of (U, D, T) alone (include/fosphor_amd_resample.h)"""
        up, down, n_taps = int(up), int(down), int(n_taps)
        span = ((Fosphor.RESAMPLE_TILE - 1) * down + up - 1) // up + n_taps // up
        return "tile" if 8 * (span + 1) + 4 * ((n_taps + 3) & ~3) <= Fosphor.RESAMPLE_TILE_LDS else "direct"

    @staticmethod
    def resample_n_out(n, up, down, n_taps, phase0=0):
        """fosphor_amd_resample_n_out: the largest valid n_out of a job of n samples, ((n - Q) U - phase0) // D + 1 or 0"""
        rv = _lib.load().fosphor_amd_resample_n_out(int(n), int(up), int(down), int(n_taps), int(phase0))
        if rv < 0:
            _fail("fosphor_amd_resample_n_out", rv, ValueError)
        return rv

    @staticmethod
    def resample_design(up, down, branch_taps, guard=0.8):
        """fosphor_amd_resample_design: the Hamming-windowed sinc prototype of branch_taps * up float32 taps for the ratio
        up / down, cutoff guard / (2 * max(up, down)) cycles per sample of the up-sampled rate; the taps sum to up and are
        symmetric; the group delay is (branch_taps * up - 1) / (2 * up) input samples"""
        out = np.empty(max(int(branch_taps), 1) * max(int(up), 1), np.float32)
        rv = _lib.load().fosphor_amd_resample_design(int(up), int(down), int(branch_taps), float(guard), out.ctypes.data)
        if rv:
            _fail("fosphor_amd_resample_design", rv, ValueError)
        return out

    @staticmethod
    def resample_ratio(rate_in, rate_out, max_term=256):
        """fosphor_amd_resample_ratio: (up, down, error): the best up / down for rate_out / rate_in with both terms at most
        min(max_term, 256), and the achieved rate's relative error (rate_in * up / down - rate_out) / rate_out"""
        up, down, err = C.c_int(0), C.c_int(0), C.c_double(0.0)
        rv = _lib.load().fosphor_amd_resample_ratio(float(rate_in), float(rate_out), int(max_term), C.byref(up), C.byref(down),
                                                    C.byref(err))
        if rv:
            _fail("fosphor_amd_resample_ratio", rv, ValueError)
        return up.value, down.value, err.value

    @staticmethod
    def resample_jobs(extract_jobs, up, down, n_taps):
        """a RESAMPLE_JOB_DTYPE array from an EXTRACT_DTYPE array (fosphor_amd_resample_from_extract: each job resamples what the
        extract job wrote, offset = out_offset, n = n_out, phase0 = 0, the largest valid n_out, the taps at taps_offset 0), the
        outputs placed back to back from out_offset 0 on"""
        L = _lib.load()
        ejobs = np.ascontiguousarray(np.atleast_1d(extract_jobs), dtype=Fosphor.EXTRACT_DTYPE)
        out = np.zeros(ejobs.size, Fosphor.RESAMPLE_JOB_DTYPE)
        at = 0
        for i, e in enumerate(ejobs):
            job = _lib.ResampleJob()
            rv = L.fosphor_amd_resample_from_extract(e.tobytes(), int(up), int(down), int(n_taps), C.byref(job))
            if rv:
                _fail("fosphor_amd_resample_from_extract", rv, ValueError)
            out[i] = (job.offset, at, job.phase0, job.n, job.n_out, job.up, job.down, job.taps_offset, job.n_taps)
            at += job.n_out
        return out

    def resample(self, d_iq, jobs, taps, n_samples=None):
        """Float32 IQ at up / down of its rate, up to 4096 jobs in one call (fosphor_amd_resample): a polyphase real FIR over
        samples that are already in device memory, "valid" outputs only, every output bit-identical to resample_host().  d_iq:
        a contiguous device tensor (complex64 or float32 pairs; what extract() wrote) or a raw device pointer with n_samples;
        jobs: a RESAMPLE_JOB_DTYPE array (resample_jobs() makes one from extract jobs; out_offset is honoured, ranges must not
        overlap); taps: float32 values (uploaded) or a float32 device tensor, addressed by the jobs' taps_offset / n_taps.
        Returns a list with one torch complex64 view per job, into one device buffer that measure(), demod() and correlate()
        read as they read extract()'s."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.RESAMPLE_JOB_DTYPE)
        n_samples = _iq_count(d_iq, n_samples, "samples")
        if hasattr(taps, "data_ptr"):
            d_taps = taps
            if d_taps.dtype != torch.float32 or not d_taps.is_cuda or not d_taps.is_contiguous():
                raise ValueError("taps must be float32 values or a contiguous float32 device tensor")
        else:
            d_taps = torch.from_numpy(_or_dummy(np.ascontiguousarray(taps, dtype=np.float32).reshape(-1))).cuda()
        cap = int((jobs["out_offset"] + jobs["n_out"]).max()) if jobs.size else 0
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 1), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()			# the taps (and the caller's samples) were written on torch's stream
        rv = self.L.fosphor_amd_resample(self.h, _ptr(d_iq), n_samples, jobs.ctypes.data, int(jobs.size), d_taps.data_ptr(),
                                         int(d_taps.numel()), d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_resample", rv, RuntimeError)
        return [d_out[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] for j in jobs]

    @staticmethod
    def resample_host(iq, jobs, taps):
        """fosphor_amd_resample_host: the same outputs on the host, no GPU.  iq: complex64 or float32 pairs; taps: float32.
        Returns a list with one complex64 array per job, views into one buffer"""
        iq = _float_pairs(iq)
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.RESAMPLE_JOB_DTYPE)
        cap = int((jobs["out_offset"] + jobs["n_out"]).max()) if jobs.size else 0
        out = np.zeros(max(cap, 1), np.complex64)
        keep = _or_dummy(iq), _or_dummy(taps)
        rv = _lib.load().fosphor_amd_resample_host(keep[0].ctypes.data, iq.size // 2, jobs.ctypes.data, int(jobs.size),
                                                   keep[1].ctypes.data, taps.size, out.ctypes.data, cap)
        if rv:
            _fail("fosphor_amd_resample_host", rv, ValueError)
        return [out[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] for j in jobs]

    def resample_stats(self):
        """fosphor_amd_resample_stats as a dict: calls, launches and jobs by form, outputs, multiply-adds (RESAMPLE_STATS)"""
        return self._stats(self.L.fosphor_amd_resample_stats, self.RESAMPLE_STATS)

    SYMBOLS_STATS = ("calls", "k_fold", "k_time", "k_pick", "k_record", "jobs_estimate", "jobs_fixed", "samples", "symbols")
    SYMBOLS_MAX_JOBS = 4096				# FOSPHOR_AMD_SYMBOLS_MAX_JOBS (include/fosphor_amd_symbols.h)
    SYMBOLS_MIN_SPS, SYMBOLS_MAX_SPS = 2, 64		# FOSPHOR_AMD_SYMBOLS_MIN_SPS, FOSPHOR_AMD_SYMBOLS_MAX_SPS
    SYMBOLS_BLOCK, SYMBOLS_TILE = 64, 4096		# FOSPHOR_AMD_SYMBOLS_BLOCK, FOSPHOR_AMD_SYMBOLS_TILE
    SYMBOLS_STAGE_SPS = 8				# FOSPHOR_AMD_SYMBOLS_STAGE_SPS
    SYMBOLS_MODES = {"estimate": 0, "fixed": 1}		# FOSPHOR_AMD_SYMBOLS_ESTIMATE, FOSPHOR_AMD_SYMBOLS_FIXED
    SYMBOLS_STATUS = {"ok": 0, "no_timing": 1}		# FOSPHOR_AMD_SYMBOLS_OK, FOSPHOR_AMD_SYMBOLS_NO_TIMING
    SYMBOLS_LDS = {"fold": 33792, "time": 2048, "pick": 31968, "record": 0}	# FOSPHOR_AMD_SYMBOLS_LDS_*
    SYMBOLS_JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("sps", "<i4"), ("mode", "<i4"),
                                  ("tau", "<f4"), ("reserved", "<i4", (2,))])
    SYMBOLS_RECORD_DTYPE = np.dtype([("n_sym", "<i4"), ("first", "<i4"), ("tau", "<f4"), ("status", "<i4"), ("mu", "<f8"),
                                     ("x_re", "<f8"), ("x_im", "<f8"), ("a0", "<f8"), ("m2", "<f8"), ("m4", "<f8"), ("z2_re", "<f8"),
                                     ("z2_im", "<f8"), ("z4_re", "<f8"), ("z4_im", "<f8")])
    SYMBOLS_VALUES = tuple(k for k, _ in _lib.SymbolsValues._fields_)

    @staticmethod
    def _symbols_mode(mode):
        if isinstance(mode, str):
            if mode not in Fosphor.SYMBOLS_MODES:
                raise ValueError("mode must be one of %s" % ", ".join(Fosphor.SYMBOLS_MODES))
            return Fosphor.SYMBOLS_MODES[mode]
        return int(mode)

    @staticmethod
    def symbols_max_out(n, sps):
        """fosphor_amd_symbols_max_out: the outputs a job of n samples reserves, n < 4 ? 0 : (n - 4) // sps + 1"""
        rv = _lib.load().fosphor_amd_symbols_max_out(int(n), int(sps))
        if rv < 0:
            _fail("fosphor_amd_symbols_max_out", rv, ValueError)
        return rv

    @staticmethod
    def symbols_twiddles(sps):
        """fosphor_amd_symbols_twiddles: the table of the pass for one sps, e^(-2 pi i k / sps) for k < sps, complex128 [sps]"""
        out = np.zeros(max(int(sps), 1), np.complex128)
        rv = _lib.load().fosphor_amd_symbols_twiddles(int(sps), out.ctypes.data)
        if rv:
            _fail("fosphor_amd_symbols_twiddles", rv, ValueError)
        return out

    @staticmethod
    def symbols_jobs(source_jobs, sps, mode="estimate", tau=0.0):
        """a SYMBOLS_JOB_DTYPE array from an EXTRACT_DTYPE or a RESAMPLE_JOB_DTYPE array (fosphor_amd_symbols_from_extract,
        fosphor_amd_symbols_from_resample: each job reads what the source job wrote, offset = out_offset, n = n_out), the reserved
        outputs placed back to back from out_offset 0 on"""
        L = _lib.load()
        src = np.atleast_1d(source_jobs)
        if src.dtype == Fosphor.RESAMPLE_JOB_DTYPE:
            make, name = L.fosphor_amd_symbols_from_resample, "fosphor_amd_symbols_from_resample"
        else:
            src = np.ascontiguousarray(src, dtype=Fosphor.EXTRACT_DTYPE)
            make, name = L.fosphor_amd_symbols_from_extract, "fosphor_amd_symbols_from_extract"
        out = np.zeros(src.size, Fosphor.SYMBOLS_JOB_DTYPE)
        code = Fosphor._symbols_mode(mode)
        at = 0
        for i, s in enumerate(src):
            job = _lib.SymbolsJob()
            rv = make(s.tobytes(), int(sps), code, float(tau), C.byref(job))
            if rv:
                _fail(name, rv, ValueError)
            out[i] = (job.offset, at, job.n, job.sps, job.mode, job.tau, (0, 0))
            at += Fosphor.symbols_max_out(job.n, job.sps)
        return out

    @staticmethod
    def _symbols_outs(jobs):
        return _outs(jobs, lambda j: Fosphor.symbols_max_out(int(j["n"]), int(j["sps"])))

    def symbols(self, d_iq, jobs, n_samples=None):
        """One record and one run of symbol-rate samples per job, up to 4096 jobs in one call (fosphor_amd_symbols): the symbol
        phase from the symbol-rate line of |y|^2 (or the job's own tau), a cubic Lagrange fractional delay and a decimation by
        sps, over float32 IQ that is already in device memory.  d_iq: a contiguous device tensor (complex64 or float32 pairs; what
        extract() or resample() wrote) or a raw device pointer with n_samples; jobs: a SYMBOLS_JOB_DTYPE array (symbols_jobs()
        makes one from extract or resample jobs; out_offset is honoured, the reserved ranges must not overlap).
        Returns (records, views): a SYMBOLS_RECORD_DTYPE array copied from the device, in job order, and a list with one torch
        complex64 view of n_sym symbols per job, into one device buffer."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.SYMBOLS_JOB_DTYPE)
        n_samples = _iq_count(d_iq, n_samples, "samples")
        _, cap = self._symbols_outs(jobs)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 1), dtype=torch.complex64, device="cuda")
        d_rec = torch.empty(max(jobs.size, 1) * self.SYMBOLS_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()			# the caller's samples were written on torch's stream
        rv = self.L.fosphor_amd_symbols(self.h, _ptr(d_iq), n_samples, jobs.ctypes.data, int(jobs.size), d_rec.data_ptr(),
                                        d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_symbols", rv, RuntimeError)
        records = d_rec.cpu().numpy().view(self.SYMBOLS_RECORD_DTYPE)[:jobs.size].copy()
        return records, [d_out[int(j["out_offset"]):int(j["out_offset"]) + int(r["n_sym"])] for j, r in zip(jobs, records)]

    @staticmethod
    def symbols_host(iq, jobs):
        """fosphor_amd_symbols_host: the same records and symbols on the host, no GPU.  iq: complex64 or float32 pairs.  Returns
        (records, views), the views complex64 arrays into one buffer"""
        iq = _float_pairs(iq)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.SYMBOLS_JOB_DTYPE)
        _, cap = Fosphor._symbols_outs(jobs)
        out = np.zeros(max(cap, 1), np.complex64)
        records = np.zeros(max(jobs.size, 1), Fosphor.SYMBOLS_RECORD_DTYPE)
        keep = _or_dummy(iq)
        rv = _lib.load().fosphor_amd_symbols_host(keep.ctypes.data, iq.size // 2, jobs.ctypes.data, int(jobs.size),
                                                  records.ctypes.data, out.ctypes.data, cap)
        if rv:
            _fail("fosphor_amd_symbols_host", rv, ValueError)
        records = records[:jobs.size]
        return records, [out[int(j["out_offset"]):int(j["out_offset"]) + int(r["n_sym"])] for j, r in zip(jobs, records)]

    @staticmethod
    def symbols_derive(records, sps, sample_rate):
        """fosphor_amd_symbols_derive per record: a list of dicts of SYMBOLS_VALUES (symbols, seconds, Hz, dB, radians).  sps: one
        value for all the records or one per record"""
        L = _lib.load()
        records = np.ascontiguousarray(np.atleast_1d(records), dtype=Fosphor.SYMBOLS_RECORD_DTYPE)
        out = []
        for r, s in zip(records, np.broadcast_to(np.asarray(sps), records.shape)):
            v = _lib.SymbolsValues()
            rv = L.fosphor_amd_symbols_derive(r.tobytes(), int(s), float(sample_rate), C.byref(v))
            if rv:
                _fail("fosphor_amd_symbols_derive", rv, ValueError)
            out.append({k: getattr(v, k) for k in Fosphor.SYMBOLS_VALUES})
        return out

    def symbols_stats(self):
        """fosphor_amd_symbols_stats as a dict: calls, launches by kernel, jobs by mode, samples, symbols (SYMBOLS_STATS)"""
        return self._stats(self.L.fosphor_amd_symbols_stats, self.SYMBOLS_STATS)

    CARRIER_STATS = ("calls", "k_lag", "k_freq", "k_sum", "k_phase", "k_turn", "jobs_freq", "jobs_phase", "symbols")
    CARRIER_MAX_JOBS = 4096				# FOSPHOR_AMD_CARRIER_MAX_JOBS (include/fosphor_amd_carrier.h)
    CARRIER_MAX_LAG = 64				# FOSPHOR_AMD_CARRIER_MAX_LAG
    CARRIER_BLOCK, CARRIER_TILE = 64, 4096		# FOSPHOR_AMD_CARRIER_BLOCK, FOSPHOR_AMD_CARRIER_TILE
    CARRIER_MODES = {"estimate": 0, "freq_fixed": 1, "phase_fixed": 2, "fixed": 3}	# sums of FOSPHOR_AMD_CARRIER_FREQ_FIXED, _PHASE_FIXED
    CARRIER_STATUS = {"ok": 0, "no_carrier": 1}		# FOSPHOR_AMD_CARRIER_OK, FOSPHOR_AMD_CARRIER_NO_CARRIER
    CARRIER_LDS = {"lag": 15536, "freq": 0, "sum": 10400, "phase": 0, "turn": 0}	# FOSPHOR_AMD_CARRIER_LDS_*
    CARRIER_JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("order", "<i4"), ("mode", "<i4"),
                                  ("lag", "<i4"), ("freq", "<f8"), ("phase", "<f8")])
    CARRIER_RECORD_DTYPE = np.dtype([("n", "<i4"), ("order", "<i4"), ("lag_used", "<i4"), ("status", "<i4"), ("freq", "<f8"),
                                     ("phase", "<f8"), ("r1_re", "<f8"), ("r1_im", "<f8"), ("rl_re", "<f8"), ("rl_im", "<f8"),
                                     ("z_re", "<f8"), ("z_im", "<f8"), ("m2", "<f8"), ("mm", "<f8")])
    CARRIER_VALUES = tuple(k for k, _ in _lib.CarrierValues._fields_)

    @staticmethod
    def _carrier_mode(mode):
        if isinstance(mode, str):
            if mode not in Fosphor.CARRIER_MODES:
                raise ValueError("mode must be one of %s" % ", ".join(Fosphor.CARRIER_MODES))
            return Fosphor.CARRIER_MODES[mode]
        return int(mode)

    @staticmethod
    def cossin_turns(t):
        """fosphor_amd_cossin_turns as the library compiled it: (cos, sin) of t turns, element-wise over float64"""
        t = np.asarray(t, np.float64)
        shape = t.shape
        t = np.ascontiguousarray(t).reshape(-1)
        c, s = np.zeros(max(t.size, 1)), np.zeros(max(t.size, 1))
        keep = t if t.size else np.zeros(1)
        rv = _lib.load().fosphor_amd_carrier_cossin_turns_n(keep.ctypes.data, int(t.size), c.ctypes.data, s.ctypes.data)
        if rv:
            _fail("fosphor_amd_carrier_cossin_turns_n", rv, ValueError)
        return c[:t.size].reshape(shape), s[:t.size].reshape(shape)

    @staticmethod
    def carrier_jobs(symbols_jobs, symbols_records, order, mode="estimate", lag=16, freq=0.0, phase=0.0):
        """a CARRIER_JOB_DTYPE array from a SYMBOLS_JOB_DTYPE array and the SYMBOLS_RECORD_DTYPE array that symbols() gave for it
        (fosphor_amd_carrier_from_symbols: each job reads what the symbols job wrote, offset = out_offset, n = n_sym), the outputs
        placed back to back from out_offset 0 on"""
        L = _lib.load()
        src = np.ascontiguousarray(np.atleast_1d(symbols_jobs), dtype=Fosphor.SYMBOLS_JOB_DTYPE)
        rec = np.ascontiguousarray(np.atleast_1d(symbols_records), dtype=Fosphor.SYMBOLS_RECORD_DTYPE)
        if src.size != rec.size:
            raise ValueError("one symbols record per symbols job")
        out = np.zeros(src.size, Fosphor.CARRIER_JOB_DTYPE)
        code = Fosphor._carrier_mode(mode)
        at = 0
        for i, (s, r) in enumerate(zip(src, rec)):
            job = _lib.CarrierJob()
            rv = L.fosphor_amd_carrier_from_symbols(s.tobytes(), r.tobytes(), int(order), code, int(lag), float(freq), float(phase),
                                                    C.byref(job))
            if rv:
                _fail("fosphor_amd_carrier_from_symbols", rv, ValueError)
            out[i] = (job.offset, at, job.n, job.order, job.mode, job.lag, job.freq, job.phase)
            at += job.n
        return out

    @staticmethod
    def _carrier_outs(jobs):
        return _outs(jobs, lambda j: int(j["n"]))

    def carrier(self, d_iq, jobs, n_samples=None):
        """One record and one run of derotated symbols per job, up to 4096 jobs in one call (fosphor_amd_carrier): the residual
        carrier frequency from the lag-1 and lag-L sums of the symbols' M-th power, the phase from the sum of the powers with that
        frequency removed, and the symbols turned back by both, over float32 symbols that are already in device memory.  d_iq: a
        contiguous device tensor (complex64 or float32 pairs; what symbols() wrote) or a raw device pointer with n_samples; jobs: a
        CARRIER_JOB_DTYPE array (carrier_jobs() makes one from symbols jobs and records; out_offset is honoured, the outputs
        must not overlap).
        Returns (records, views): a CARRIER_RECORD_DTYPE array copied from the device, in job order, and a list with one torch
        complex64 view per job into one device buffer, n symbols long, or empty where the record says no_carrier."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.CARRIER_JOB_DTYPE)
        n_samples = _iq_count(d_iq, n_samples, "samples")
        _, cap = self._carrier_outs(jobs)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 1), dtype=torch.complex64, device="cuda")
        d_rec = torch.empty(max(jobs.size, 1) * self.CARRIER_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()			# the caller's symbols were written on torch's stream
        rv = self.L.fosphor_amd_carrier(self.h, _ptr(d_iq), n_samples, jobs.ctypes.data, int(jobs.size), d_rec.data_ptr(),
                                        d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_carrier", rv, RuntimeError)
        records = d_rec.cpu().numpy().view(self.CARRIER_RECORD_DTYPE)[:jobs.size].copy()
        return records, [d_out[int(j["out_offset"]):int(j["out_offset"]) + (int(j["n"]) if r["status"] == 0 else 0)]
                         for j, r in zip(jobs, records)]

    @staticmethod
    def carrier_host(iq, jobs):
        """fosphor_amd_carrier_host: the same records and symbols on the host, no GPU.  iq: complex64 or float32 pairs.  Returns
        (records, views), the views complex64 arrays into one buffer"""
        iq = _float_pairs(iq)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.CARRIER_JOB_DTYPE)
        _, cap = Fosphor._carrier_outs(jobs)
        out = np.zeros(max(cap, 1), np.complex64)
        records = np.zeros(max(jobs.size, 1), Fosphor.CARRIER_RECORD_DTYPE)
        keep = _or_dummy(iq)
        rv = _lib.load().fosphor_amd_carrier_host(keep.ctypes.data, iq.size // 2, jobs.ctypes.data, int(jobs.size),
                                                  records.ctypes.data, out.ctypes.data, cap)
        if rv:
            _fail("fosphor_amd_carrier_host", rv, ValueError)
        records = records[:jobs.size]
        return records, [out[int(j["out_offset"]):int(j["out_offset"]) + (int(j["n"]) if r["status"] == 0 else 0)]
                         for j, r in zip(jobs, records)]

    @staticmethod
    def carrier_derive(records, symbol_rate):
        """fosphor_amd_carrier_derive per record: a list of dicts of CARRIER_VALUES (Hz, radians, ratios)"""
        L = _lib.load()
        records = np.ascontiguousarray(np.atleast_1d(records), dtype=Fosphor.CARRIER_RECORD_DTYPE)
        out = []
        for r in records:
            v = _lib.CarrierValues()
            rv = L.fosphor_amd_carrier_derive(r.tobytes(), float(symbol_rate), C.byref(v))
            if rv:
                _fail("fosphor_amd_carrier_derive", rv, ValueError)
            out.append({k: getattr(v, k) for k in Fosphor.CARRIER_VALUES})
        return out

    def carrier_stats(self):
        """fosphor_amd_carrier_stats as a dict: calls, launches by kernel, jobs that estimate frequency and phase, symbols
        (CARRIER_STATS)"""
        return self._stats(self.L.fosphor_amd_carrier_stats, self.CARRIER_STATS)

    DECIDE_STATS = ("calls", "k_hard", "k_uw", "k_job", "k_out", "jobs_uw", "symbols")
    DECIDE_MAX_JOBS = 4096				# FOSPHOR_AMD_DECIDE_MAX_JOBS (include/fosphor_amd_decide.h)
    DECIDE_MAX_UW, DECIDE_MAX_UW_TABLE = 64, 65536	# FOSPHOR_AMD_DECIDE_MAX_UW, FOSPHOR_AMD_DECIDE_MAX_UW_TABLE
    DECIDE_BLOCK, DECIDE_TILE = 64, 4096		# FOSPHOR_AMD_DECIDE_BLOCK, FOSPHOR_AMD_DECIDE_TILE
    DECIDE_UW_GROUP = 256				# FOSPHOR_AMD_DECIDE_UW_GROUP
    DECIDE_FLAGS = {"diff": 1, "gray": 2, "uw": 4}	# FOSPHOR_AMD_DECIDE_DIFF, _GRAY, _UW
    DECIDE_STATUS = {"ok": 0, "no_uw": 1}		# FOSPHOR_AMD_DECIDE_OK, FOSPHOR_AMD_DECIDE_NO_UW
    DECIDE_LDS = {"hard": 7904, "uw": 752, "job": 0, "out": 0}	# FOSPHOR_AMD_DECIDE_LDS_*
    DECIDE_JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("order", "<i4"), ("flags", "<i4"),
                                 ("uw_offset", "<i4"), ("uw_len", "<i4"), ("uw_first", "<i4"), ("uw_count", "<i4"),
                                 ("uw_max_errors", "<i4"), ("reserved", "<i4", (4,))])
    DECIDE_RECORD_DTYPE = np.dtype([("n", "<i4"), ("order", "<i4"), ("flags", "<i4"), ("status", "<i4"), ("uw_pos", "<i4"),
                                    ("uw_rot", "<i4"), ("uw_errors", "<i4"), ("erasures", "<i4"), ("a", "<f8"), ("b", "<f8"),
                                    ("m2", "<f8"), ("hist", "<i4", (8,)), ("reserved", "<i4", (2,))])
    DECIDE_VALUES = tuple(k for k, _ in _lib.DecideValues._fields_)

    @staticmethod
    def _decide_flags(flags):
        """an integer, one name of DECIDE_FLAGS or several ("diff", "uw") -> the sum of the bits"""
        if isinstance(flags, str):
            flags = (flags,)
        if isinstance(flags, (tuple, list, set, frozenset)):
            for k in flags:
                if k not in Fosphor.DECIDE_FLAGS:
                    raise ValueError("flags must be of %s" % ", ".join(Fosphor.DECIDE_FLAGS))
            return sum(Fosphor.DECIDE_FLAGS[k] for k in set(flags))
        return int(flags)

    @staticmethod
    def decide_owned(n):
        """the bytes a job of n symbols owns in d_out: 4 ceil(n / 4)"""
        return 4 * ((int(n) + 3) // 4)

    @staticmethod
    def decide_jobs(carrier_jobs, carrier_records, flags=0, uw_offset=0, uw_len=0, uw_first=0, uw_count=0, uw_max_errors=0, gap=4):
        """a DECIDE_JOB_DTYPE array from a CARRIER_JOB_DTYPE array and the CARRIER_RECORD_DTYPE array that carrier() gave for it
        (fosphor_amd_decide_from_carrier: each job reads what the carrier job wrote, offset = out_offset, n and order the
        record's, n = 0 where the record says no_carrier), the owned bytes placed from out_offset 0 on at multiples of 4 with
        `gap` bytes (rounded up to a multiple of 4) between them"""
        L = _lib.load()
        src = np.ascontiguousarray(np.atleast_1d(carrier_jobs), dtype=Fosphor.CARRIER_JOB_DTYPE)
        rec = np.ascontiguousarray(np.atleast_1d(carrier_records), dtype=Fosphor.CARRIER_RECORD_DTYPE)
        if src.size != rec.size:
            raise ValueError("one carrier record per carrier job")
        if gap < 0:
            raise ValueError("gap must be >= 0")
        out = np.zeros(src.size, Fosphor.DECIDE_JOB_DTYPE)
        code = Fosphor._decide_flags(flags)
        at = 0
        for i, (s, r) in enumerate(zip(src, rec)):
            job = _lib.DecideJob()
            rv = L.fosphor_amd_decide_from_carrier(s.tobytes(), r.tobytes(), code, int(uw_offset), int(uw_len), int(uw_first),
                                                   int(uw_count), int(uw_max_errors), C.byref(job))
            if rv:
                _fail("fosphor_amd_decide_from_carrier", rv, ValueError)
            out[i] = (job.offset, at, job.n, job.order, job.flags, job.uw_offset, job.uw_len, job.uw_first, job.uw_count,
                      job.uw_max_errors, (0, 0, 0, 0))
            at += Fosphor.decide_owned(job.n) + Fosphor.decide_owned(gap)
        return out

    @staticmethod
    def _decide_outs(jobs):
        return _outs(jobs, lambda j: Fosphor.decide_owned(j["n"]))

    @staticmethod
    def _decide_word(uw):
        """the call's unique-word table -> (a contiguous uint8 array or None, its length)"""
        if uw is None:
            return None, 0
        uw = np.ascontiguousarray(uw, dtype=np.uint8).reshape(-1)
        return (uw, int(uw.size)) if uw.size else (None, 0)

    def decide(self, d_iq, jobs, uw=None, n_samples=None):
        """One record and one byte per symbol per job, up to 4096 jobs in one call (fosphor_amd_decide): the nearest of M PSK points
        per symbol, the 1 / M ambiguity taken out by differential decoding or by the rotation under which a unique word is found,
        optional Gray demapping, over float32 symbols that are already in device memory.  d_iq: a contiguous device tensor
        (complex64 or float32 pairs; what carrier() wrote) or a raw device pointer with n_samples; jobs: a DECIDE_JOB_DTYPE array
        (decide_jobs() makes one from carrier jobs and records; out_offset is honoured, the owned bytes must not overlap); uw: the
        call's table of unique-word symbols, uint8, that the jobs' uw_offset point into.
        Returns (records, views): a DECIDE_RECORD_DTYPE array copied from the device, in job order, and a list with one torch
        uint8 view of n symbols per job into one device buffer."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.DECIDE_JOB_DTYPE)
        n_samples = _iq_count(d_iq, n_samples, "samples")
        uw, n_uw = self._decide_word(uw)
        _, cap = self._decide_outs(jobs)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 4), dtype=torch.uint8, device="cuda")
        d_rec = torch.empty(max(jobs.size, 1) * self.DECIDE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()			# the caller's symbols were written on torch's stream
        rv = self.L.fosphor_amd_decide(self.h, _ptr(d_iq), n_samples, jobs.ctypes.data, int(jobs.size),
                                       uw.ctypes.data if n_uw else None, n_uw, d_rec.data_ptr(), d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_decide", rv, RuntimeError)
        records = d_rec.cpu().numpy().view(self.DECIDE_RECORD_DTYPE)[:jobs.size].copy()
        return records, [d_out[int(j["out_offset"]):int(j["out_offset"]) + int(j["n"])] for j in jobs]

    @staticmethod
    def decide_host(iq, jobs, uw=None):
        """fosphor_amd_decide_host: the same records and bytes on the host, no GPU.  iq: complex64 or float32 pairs.  Returns
        (records, views), the views uint8 arrays into one buffer"""
        iq = _float_pairs(iq)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.DECIDE_JOB_DTYPE)
        uw, n_uw = Fosphor._decide_word(uw)
        _, cap = Fosphor._decide_outs(jobs)
        out = np.zeros(max(cap, 4) // 4, np.uint32).view(np.uint8)
        records = np.zeros(max(jobs.size, 1), Fosphor.DECIDE_RECORD_DTYPE)
        keep = _or_dummy(iq)
        rv = _lib.load().fosphor_amd_decide_host(keep.ctypes.data, iq.size // 2, jobs.ctypes.data, int(jobs.size),
                                                 uw.ctypes.data if n_uw else None, n_uw, records.ctypes.data, out.ctypes.data, cap)
        if rv:
            _fail("fosphor_amd_decide_host", rv, ValueError)
        return records[:jobs.size], [out[int(j["out_offset"]):int(j["out_offset"]) + int(j["n"])] for j in jobs]

    @staticmethod
    def decide_derive(records, uw_len=0):
        """fosphor_amd_decide_derive per record: a list of dicts of DECIDE_VALUES (ratios, dB, radians).  uw_len: one value for all
        the records or one per record, the jobs' (0 without a unique word)"""
        L = _lib.load()
        records = np.ascontiguousarray(np.atleast_1d(records), dtype=Fosphor.DECIDE_RECORD_DTYPE)
        out = []
        for r, u in zip(records, np.broadcast_to(np.asarray(uw_len), records.shape)):
            v = _lib.DecideValues()
            rv = L.fosphor_amd_decide_derive(r.tobytes(), int(u), C.byref(v))
            if rv:
                _fail("fosphor_amd_decide_derive", rv, ValueError)
            out.append({k: getattr(v, k) for k in Fosphor.DECIDE_VALUES})
        return out

    def decide_stats(self):
        """fosphor_amd_decide_stats as a dict: calls, launches by kernel, jobs with a unique word, symbols (DECIDE_STATS)"""
        return self._stats(self.L.fosphor_amd_decide_stats, self.DECIDE_STATS)

    DECODE_STATS = ("calls", "k_bits", "k_acs", "k_trace", "k_rec", "jobs_crc", "steps")
    DECODE_MAX_JOBS = 4096				# FOSPHOR_AMD_DECODE_MAX_JOBS (include/fosphor_amd_decode.h)
    DECODE_MAX_STEPS, DECODE_MAX_CALL_STEPS = 65536, 1 << 22	# FOSPHOR_AMD_DECODE_MAX_STEPS, FOSPHOR_AMD_DECODE_MAX_CALL_STEPS
    DECODE_BLOCK, DECODE_INF = 64, 1 << 24		# FOSPHOR_AMD_DECODE_BLOCK, FOSPHOR_AMD_DECODE_INF
    DECODE_FLAGS = {"terminated": 1}			# FOSPHOR_AMD_DECODE_TERMINATED
    DECODE_STATUS = {"ok": 0, "crc_fail": 1, "short": 2}	# FOSPHOR_AMD_DECODE_OK, _CRC_FAIL, _SHORT
    DECODE_LDS = {"bits": 0, "acs": 0, "trace": 0, "rec": 0}	# FOSPHOR_AMD_DECODE_LDS_*
    DECODE_JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("order", "<i4"), ("steps", "<i4"),
                                 ("flags", "<i4"), ("k", "u1"), ("n_poly", "u1"), ("period", "u1"), ("crc_width", "u1"),
                                 ("polys", "<u2", (3,)), ("punct", "<u2", (3,)), ("crc_poly", "<u4"), ("crc_init", "<u4"),
                                 ("crc_xorout", "<u4"), ("reserved", "<u4")])
    DECODE_RECORD_DTYPE = np.dtype([("n_steps", "<i4"), ("n_bits", "<i4"), ("n_coded", "<i4"), ("status", "<i4"),
                                    ("end_state", "<i4"), ("metric", "<i4"), ("best_state", "<i4"), ("best_metric", "<i4"),
                                    ("crc_calc", "<u4"), ("crc_recv", "<u4"), ("k", "<i4"), ("flags", "<i4"),
                                    ("reserved", "<i4", (4,))])
    DECODE_VALUES = tuple(k for k, _ in _lib.DecodeValues._fields_)

    @staticmethod
    def decode_steps(n, order, n_poly=2, period=1, punct=(1, 1, 0)):
        """fosphor_amd_decode_steps: the trellis steps that n symbols of order M hold under the puncture masks (rule 2's T for
        steps = 0)"""
        p = np.ascontiguousarray(punct, dtype=np.uint16)
        if p.size != 3:
            raise ValueError("punct holds three masks")
        rv = _lib.load().fosphor_amd_decode_steps(int(n), int(order), int(n_poly), int(period), p.ctypes.data)
        if rv < 0:
            _fail("fosphor_amd_decode_steps", rv, ValueError)
        return rv

    @staticmethod
    def _decode_shape(j):
        """(T, n_bits) of a job as rules 2 and 5 give them; raises ValueError where rule 9 refuses the pattern"""
        T = int(j["steps"]) or Fosphor.decode_steps(j["n"], j["order"], j["n_poly"], j["period"], j["punct"])
        return T, (max(T - (int(j["k"]) - 1), 0) if int(j["flags"]) & 1 else T)

    @staticmethod
    def decode_owned(n_bits):
        """the bytes a job of n_bits decoded bits owns in d_out: 8 ceil(n_bits / 64)"""
        return 8 * ((int(n_bits) + 63) // 64)

    @staticmethod
    def decode_jobs(decide_jobs, decide_records, uw_len, n_payload=0, k=7, polys=(0o171, 0o133, 0), period=1, punct=(1, 1, 0),
                    steps=0, flags=0, crc_width=0, crc_poly=0, crc_init=0, crc_xorout=0, gap=8):
        """a DECODE_JOB_DTYPE array from a DECIDE_JOB_DTYPE array and the DECIDE_RECORD_DTYPE array that decide() gave for it
        (fosphor_amd_decode_from_decide: each job reads what the decide job wrote behind its unique word, n = n_payload symbols
        or all of them, n = 0 where the record says no_uw), the code, the puncture masks and the CRC the same for every job, the
        owned bytes placed from out_offset 0 on at multiples of 8 with `gap` bytes (rounded up to a multiple of 8) between them"""
        L = _lib.load()
        src = np.ascontiguousarray(np.atleast_1d(decide_jobs), dtype=Fosphor.DECIDE_JOB_DTYPE)
        rec = np.ascontiguousarray(np.atleast_1d(decide_records), dtype=Fosphor.DECIDE_RECORD_DTYPE)
        if src.size != rec.size:
            raise ValueError("one decide record per decide job")
        if gap < 0:
            raise ValueError("gap must be >= 0")
        if isinstance(flags, str):
            if flags not in Fosphor.DECODE_FLAGS:
                raise ValueError("flags must be of %s" % ", ".join(Fosphor.DECODE_FLAGS))
            flags = Fosphor.DECODE_FLAGS[flags]
        out = np.zeros(src.size, Fosphor.DECODE_JOB_DTYPE)
        n_poly = 3 if len(polys) > 2 and polys[2] else 2
        at = 0
        for i, (s, r) in enumerate(zip(src, rec)):
            job = _lib.DecodeJob()
            rv = L.fosphor_amd_decode_from_decide(s.tobytes(), r.tobytes(), int(uw_len), int(n_payload), C.byref(job))
            if rv:
                _fail("fosphor_amd_decode_from_decide", rv, ValueError)
            o = out[i]
            o["offset"], o["out_offset"], o["n"], o["order"], o["steps"], o["flags"] = job.offset, at, job.n, job.order, steps, flags
            o["k"], o["n_poly"], o["period"], o["crc_width"] = k, n_poly, period, crc_width
            o["polys"], o["punct"] = tuple(polys) + (0,) * (3 - len(polys)), tuple(punct) + (0,) * (3 - len(punct))
            o["crc_poly"], o["crc_init"], o["crc_xorout"] = crc_poly, crc_init, crc_xorout
            at += Fosphor.decode_owned(Fosphor._decode_shape(o)[1]) + 8 * ((int(gap) + 7) // 8)
        return out

    @staticmethod
    def _decode_outs(jobs):
        """(n_bits per job, the capacity the jobs need); a job that rule 9 will refuse counts as owning nothing"""
        def bits(j):
            try:
                return Fosphor._decode_shape(j)[1]
            except ValueError:
                return 0
        n_bits = [bits(j) for j in jobs]
        return n_bits, max([int(j["out_offset"]) + Fosphor.decode_owned(b) for j, b in zip(jobs, n_bits)] + [0])

    def decode(self, d_sym, jobs, n_bytes=None):
        """One record and the decoded bits per job, up to 4096 jobs in one call (fosphor_amd_decode): the symbols' bits
        depunctured, a Viterbi decoder over the whole frame with one lane per state, the decoded bits packed MSB first and a CRC
        over them, over one byte per symbol that is already in device memory.  d_sym: a contiguous uint8 device tensor (what
        decide() wrote) or a raw device pointer with n_bytes; jobs: a DECODE_JOB_DTYPE array (decode_jobs() makes one from decide
        jobs and records; out_offset is honoured, the owned bytes must not overlap).
        Returns (records, views): a DECODE_RECORD_DTYPE array copied from the device, in job order, and a list with one torch
        uint8 view of ceil(n_bits / 8) bytes per job into one device buffer."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.DECODE_JOB_DTYPE)
        if n_bytes is None:
            if not hasattr(d_sym, "numel"):
                raise ValueError("a raw device pointer needs n_bytes")
            if str(d_sym.dtype) != "torch.uint8" or not d_sym.is_contiguous():
                raise ValueError("d_sym must be a contiguous uint8 tensor")
            n_bytes = d_sym.numel()
        _, cap = self._decode_outs(jobs)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 8) // 8, dtype=torch.int64, device="cuda").view(torch.uint8)
        d_rec = torch.empty(max(jobs.size, 1) * self.DECODE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()			# the caller's bytes were written on torch's stream
        rv = self.L.fosphor_amd_decode(self.h, _ptr(d_sym), int(n_bytes), jobs.ctypes.data, int(jobs.size), d_rec.data_ptr(),
                                       d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_decode", rv, RuntimeError)
        records = d_rec.cpu().numpy().view(self.DECODE_RECORD_DTYPE)[:jobs.size].copy()
        return records, [d_out[int(j["out_offset"]):int(j["out_offset"]) + (int(r["n_bits"]) + 7) // 8] for j, r in zip(jobs, records)]

    @staticmethod
    def decode_host(sym, jobs):
        """fosphor_amd_decode_host: the same records and bits on the host, no GPU.  sym: uint8, one symbol a byte.  Returns
        (records, views), the views uint8 arrays of ceil(n_bits / 8) bytes into one buffer"""
        sym = np.ascontiguousarray(sym, dtype=np.uint8).reshape(-1)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.DECODE_JOB_DTYPE)
        _, cap = Fosphor._decode_outs(jobs)
        out = np.zeros(max(cap, 8) // 8, np.uint64).view(np.uint8)
        records = np.zeros(max(jobs.size, 1), Fosphor.DECODE_RECORD_DTYPE)
        keep = sym if sym.size else np.zeros(8, np.uint8)
        rv = _lib.load().fosphor_amd_decode_host(keep.ctypes.data, int(sym.size), jobs.ctypes.data, int(jobs.size),
                                                 records.ctypes.data, out.ctypes.data, cap)
        if rv:
            _fail("fosphor_amd_decode_host", rv, ValueError)
        records = records[:jobs.size]
        return records, [out[int(j["out_offset"]):int(j["out_offset"]) + (int(r["n_bits"]) + 7) // 8] for j, r in zip(jobs, records)]

    @staticmethod
    def decode_derive(records):
        """fosphor_amd_decode_derive per record: a list of dicts of DECODE_VALUES (ratios)"""
        L = _lib.load()
        records = np.ascontiguousarray(np.atleast_1d(records), dtype=Fosphor.DECODE_RECORD_DTYPE)
        out = []
        for r in records:
            v = _lib.DecodeValues()
            rv = L.fosphor_amd_decode_derive(r.tobytes(), C.byref(v))
            if rv:
                _fail("fosphor_amd_decode_derive", rv, ValueError)
            out.append({k: getattr(v, k) for k in Fosphor.DECODE_VALUES})
        return out

    def decode_stats(self):
        """fosphor_amd_decode_stats as a dict: calls, launches by kernel, jobs with a CRC, steps (DECODE_STATS)"""
        return self._stats(self.L.fosphor_amd_decode_stats, self.DECODE_STATS)

    SOFT_STATS = ("calls", "k_bits", "k_acs", "k_trace", "k_rec", "jobs_crc", "steps")
    SOFT_MAX_JOBS = 4096				# FOSPHOR_AMD_SOFT_MAX_JOBS (include/fosphor_amd_soft.h)
    SOFT_MAX_STEPS, SOFT_MAX_CALL_STEPS = 65536, 1 << 22	# FOSPHOR_AMD_SOFT_MAX_STEPS, FOSPHOR_AMD_SOFT_MAX_CALL_STEPS
    SOFT_BLOCK, SOFT_GROUP = 64, 256			# FOSPHOR_AMD_SOFT_BLOCK, FOSPHOR_AMD_SOFT_GROUP
    SOFT_MAX_VALUE, SOFT_INF = 127, 1 << 25		# FOSPHOR_AMD_SOFT_MAX_VALUE, FOSPHOR_AMD_SOFT_INF
    SOFT_FLAGS = {"terminated": 1, "gray": 2}		# FOSPHOR_AMD_SOFT_TERMINATED, FOSPHOR_AMD_SOFT_GRAY
    SOFT_STATUS = {"ok": 0, "crc_fail": 1, "short": 2}	# FOSPHOR_AMD_SOFT_OK, _CRC_FAIL, _SHORT
    SOFT_LDS = {"bits": 32, "acs": 0, "trace": 0, "rec": 0}	# FOSPHOR_AMD_SOFT_LDS_*
    SOFT_JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("order", "<i2"), ("flags", "<i2"),
                               ("steps", "<i4"), ("k", "u1"), ("n_poly", "u1"), ("period", "u1"), ("crc_width", "u1"),
                               ("polys", "<u2", (3,)), ("punct", "<u2", (3,)), ("crc_poly", "<u4"), ("crc_init", "<u4"),
                               ("crc_xorout", "<u4"), ("rot", "<i4"), ("scale", "<f4")])
    SOFT_RECORD_DTYPE = np.dtype([("n_steps", "<i4"), ("n_bits", "<i4"), ("n_coded", "<i4"), ("status", "<i4"),
                                  ("end_state", "<i4"), ("metric", "<i4"), ("best_state", "<i4"), ("best_metric", "<i4"),
                                  ("crc_calc", "<u4"), ("crc_recv", "<u4"), ("k", "<i4"), ("flags", "<i4"),
                                  ("erasures", "<i4"), ("saturated", "<i4"), ("abs_sum", "<i8")])
    SOFT_VALUES = tuple(k for k, _ in _lib.SoftValues._fields_)

    @staticmethod
    def _soft_flags(flags):
        """an integer, one name of SOFT_FLAGS or several ("terminated", "gray") -> the sum of the bits"""
        if isinstance(flags, str):
            flags = (flags,)
        if isinstance(flags, (tuple, list, set, frozenset)):
            for k in flags:
                if k not in Fosphor.SOFT_FLAGS:
                    raise ValueError("flags must be of %s" % ", ".join(Fosphor.SOFT_FLAGS))
            return sum(Fosphor.SOFT_FLAGS[k] for k in set(flags))
        return int(flags)

    @staticmethod
    def soft_jobs(decide_jobs, decide_records, uw_len, n_payload=0, k=7, polys=(0o171, 0o133, 0), period=1, punct=(1, 1, 0),
                  steps=0, flags=0, crc_width=0, crc_poly=0, crc_init=0, crc_xorout=0, gap=8):
        """a SOFT_JOB_DTYPE array from a DECIDE_JOB_DTYPE array and the DECIDE_RECORD_DTYPE array that decide() gave for it
        (fosphor_amd_soft_from_decide: each job reads the symbols that the decide job read, behind its unique word, n = n_payload
        symbols or all of them, n = 0 where the record says no_uw; rot is the record's uw_rot, scale 16 n / a, "gray" the decide
        job's), the code, the puncture masks and the CRC the same for every job, `flags` ("terminated") added to what the decide
        job gives, the owned bytes placed from out_offset 0 on at multiples of 8 with `gap` bytes (rounded up to a multiple of 8)
        between them"""
        L = _lib.load()
        src = np.ascontiguousarray(np.atleast_1d(decide_jobs), dtype=Fosphor.DECIDE_JOB_DTYPE)
        rec = np.ascontiguousarray(np.atleast_1d(decide_records), dtype=Fosphor.DECIDE_RECORD_DTYPE)
        if src.size != rec.size:
            raise ValueError("one decide record per decide job")
        if gap < 0:
            raise ValueError("gap must be >= 0")
        flags = Fosphor._soft_flags(flags)
        out = np.zeros(src.size, Fosphor.SOFT_JOB_DTYPE)
        n_poly = 3 if len(polys) > 2 and polys[2] else 2
        at = 0
        for i, (s, r) in enumerate(zip(src, rec)):
            job = _lib.SoftJob()
            rv = L.fosphor_amd_soft_from_decide(s.tobytes(), r.tobytes(), int(uw_len), int(n_payload), C.byref(job))
            if rv:
                _fail("fosphor_amd_soft_from_decide", rv, ValueError)
            o = out[i]
            o["offset"], o["out_offset"], o["n"], o["order"], o["steps"], o["flags"] = job.offset, at, job.n, job.order, steps, job.flags | flags
            o["k"], o["n_poly"], o["period"], o["crc_width"] = k, n_poly, period, crc_width
            o["polys"], o["punct"] = tuple(polys) + (0,) * (3 - len(polys)), tuple(punct) + (0,) * (3 - len(punct))
            o["crc_poly"], o["crc_init"], o["crc_xorout"] = crc_poly, crc_init, crc_xorout
            o["rot"], o["scale"] = job.rot, job.scale
            at += Fosphor.decode_owned(Fosphor._decode_shape(o)[1]) + 8 * ((int(gap) + 7) // 8)
        return out

    def soft(self, d_iq, jobs, n_samples=None):
        """One record and the decoded bits per job, up to 4096 jobs in one call (fosphor_amd_soft): one quantised soft value per
        coded bit from the derotated symbols, depunctured, a soft-input Viterbi decoder over the whole frame with one lane per
        state, the decoded bits packed MSB first and a CRC over them, over float32 symbols that are already in device memory.
        d_iq: a contiguous device tensor (complex64 or float32 pairs; what carrier() wrote and decide() read) or a raw device
        pointer with n_samples; jobs: a SOFT_JOB_DTYPE array (soft_jobs() makes one from decide jobs and records; out_offset is
        honoured, the owned bytes must not overlap).
        Returns (records, views): a SOFT_RECORD_DTYPE array copied from the device, in job order, and a list with one torch
        uint8 view of ceil(n_bits / 8) bytes per job into one device buffer."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.SOFT_JOB_DTYPE)
        n_samples = _iq_count(d_iq, n_samples, "samples")
        _, cap = self._decode_outs(jobs)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 8) // 8, dtype=torch.int64, device="cuda").view(torch.uint8)
        d_rec = torch.empty(max(jobs.size, 1) * self.SOFT_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()			# the caller's symbols were written on torch's stream
        rv = self.L.fosphor_amd_soft(self.h, _ptr(d_iq), n_samples, jobs.ctypes.data, int(jobs.size), d_rec.data_ptr(),
                                     d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_soft", rv, RuntimeError)
        records = d_rec.cpu().numpy().view(self.SOFT_RECORD_DTYPE)[:jobs.size].copy()
        return records, [d_out[int(j["out_offset"]):int(j["out_offset"]) + (int(r["n_bits"]) + 7) // 8] for j, r in zip(jobs, records)]

    @staticmethod
    def soft_host(iq, jobs):
        """fosphor_amd_soft_host: the same records and bits on the host, no GPU.  iq: complex64 or float32 pairs.  Returns
        (records, views), the views uint8 arrays of ceil(n_bits / 8) bytes into one buffer"""
        iq = _float_pairs(iq)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.SOFT_JOB_DTYPE)
        _, cap = Fosphor._decode_outs(jobs)
        out = np.zeros(max(cap, 8) // 8, np.uint64).view(np.uint8)
        records = np.zeros(max(jobs.size, 1), Fosphor.SOFT_RECORD_DTYPE)
        keep = _or_dummy(iq)
        rv = _lib.load().fosphor_amd_soft_host(keep.ctypes.data, iq.size // 2, jobs.ctypes.data, int(jobs.size),
                                               records.ctypes.data, out.ctypes.data, cap)
        if rv:
            _fail("fosphor_amd_soft_host", rv, ValueError)
        records = records[:jobs.size]
        return records, [out[int(j["out_offset"]):int(j["out_offset"]) + (int(r["n_bits"]) + 7) // 8] for j, r in zip(jobs, records)]

    @staticmethod
    def soft_derive(records):
        """fosphor_amd_soft_derive per record: a list of dicts of SOFT_VALUES (ratios)"""
        L = _lib.load()
        records = np.ascontiguousarray(np.atleast_1d(records), dtype=Fosphor.SOFT_RECORD_DTYPE)
        out = []
        for r in records:
            v = _lib.SoftValues()
            rv = L.fosphor_amd_soft_derive(r.tobytes(), C.byref(v))
            if rv:
                _fail("fosphor_amd_soft_derive", rv, ValueError)
            out.append({k: getattr(v, k) for k in Fosphor.SOFT_VALUES})
        return out

    def soft_stats(self):
        """fosphor_amd_soft_stats as a dict: calls, launches by kernel, jobs with a CRC, steps (SOFT_STATS)"""
        return self._stats(self.L.fosphor_amd_soft_stats, self.SOFT_STATS)

    RS_STATS = ("calls", "k_syn", "k_fix", "k_out", "k_rec", "codewords", "clean", "failed")
    RS_MAX_JOBS = 4096					# FOSPHOR_AMD_RS_MAX_JOBS (include/fosphor_amd_rs.h)
    RS_MAX_ROOTS, RS_MAX_DEPTH = 32, 16			# FOSPHOR_AMD_RS_MAX_ROOTS, FOSPHOR_AMD_RS_MAX_DEPTH
    RS_MAX_CALL_CODEWORDS = 65536			# FOSPHOR_AMD_RS_MAX_CALL_CODEWORDS
    RS_FLAGS = {"descramble_in": 1, "descramble_out": 2}	# FOSPHOR_AMD_RS_DESCRAMBLE_IN, _DESCRAMBLE_OUT
    RS_STATUS = {"ok": 0, "fail": 1}			# FOSPHOR_AMD_RS_OK, _FAIL
    RS_FAILED = 255					# FOSPHOR_AMD_RS_FAILED
    RS_LDS = {"syn": 0, "fix": 0, "out": 0, "rec": 0}	# FOSPHOR_AMD_RS_LDS_*
    RS_JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("flags", "<i4"), ("gf_poly", "<u2"), ("fcr", "u1"),
                             ("prim", "u1"), ("n_roots", "u1"), ("n_code", "u1"), ("depth", "u1"), ("scr_width", "u1"),
                             ("scr_taps", "<u4"), ("scr_init", "<u4"), ("reserved", "<u4", (7,))])
    RS_RECORD_DTYPE = np.dtype([("n_codewords", "<i4"), ("n_data", "<i4"), ("status", "<i4"), ("n_failed", "<i4"),
                                ("n_clean", "<i4"), ("corrected_symbols", "<i4"), ("corrected_bits", "<i4"), ("max_errors", "<i4"),
                                ("failed_mask", "<u4"), ("errors", "u1", (16,)), ("n_code", "<u2"), ("n_roots", "<u2"),
                                ("reserved", "<u4", (2,))])
    RS_VALUES = tuple(k for k, _ in _lib.RsValues._fields_)
    RS_CCSDS = dict(gf_poly=0x187, fcr=112, prim=11, n_roots=32)		# RS(255,223), conventional basis
    RS_DVB = dict(gf_poly=0x11d, fcr=0, prim=1, n_roots=16)			# RS(204,188)

    @staticmethod
    def _rs_flags(flags):
        if isinstance(flags, str):
            if flags not in Fosphor.RS_FLAGS:
                raise ValueError("flags must be of %s" % ", ".join(Fosphor.RS_FLAGS))
            return Fosphor.RS_FLAGS[flags]
        return int(flags)

    @staticmethod
    def rs_owned(n_data):
        """the bytes a job of n_data data bytes owns in d_out: 8 ceil(n_data / 8)"""
        return 8 * ((int(n_data) + 7) // 8)

    @staticmethod
    def _rs_n_data(j):
        return int(j["depth"]) * max(int(j["n_code"]) - int(j["n_roots"]), 0)

    @staticmethod
    def rs_jobs(out_offsets, n_bits, n_code, depth=1, skip_bytes=0, gf_poly=0x11d, fcr=0, prim=1, n_roots=16, flags=0, scr_width=0,
                scr_taps=0, scr_init=0, gap=8):
        """an RS_JOB_DTYPE array over what decode() or soft() wrote (fosphor_amd_rs_from_decode): out_offsets the decode or soft
        jobs' out_offset, n_bits their records' n_bits; each frame of depth * n_code bytes begins skip_bytes behind its job's first
        output byte and must be covered by n_bits.  The code (RS_CCSDS and RS_DVB hold two) and the scrambler are the same for
        every job, the owned bytes placed from out_offset 0 on at multiples of 8 with `gap` bytes (rounded up to a multiple of 8)
        between them"""
        L = _lib.load()
        offs = np.atleast_1d(np.asarray(out_offsets, dtype=np.int64))
        bits = np.atleast_1d(np.asarray(n_bits, dtype=np.int64))
        if offs.size != bits.size:
            raise ValueError("one n_bits per out_offset")
        if gap < 0:
            raise ValueError("gap must be >= 0")
        flags = Fosphor._rs_flags(flags)
        out = np.zeros(offs.size, Fosphor.RS_JOB_DTYPE)
        at = 0
        for i, (o, b) in enumerate(zip(offs, bits)):
            job = _lib.RsJob()
            rv = L.fosphor_amd_rs_from_decode(int(o), int(min(b, 2 ** 31 - 1)), int(skip_bytes), int(n_code), int(depth), C.byref(job))
            if rv:
                _fail("fosphor_amd_rs_from_decode", rv, ValueError)
            j = out[i]
            j["offset"], j["out_offset"], j["flags"], j["n_code"], j["depth"] = job.offset, at, flags, job.n_code, job.depth
            j["gf_poly"], j["fcr"], j["prim"], j["n_roots"] = gf_poly, fcr, prim, n_roots
            j["scr_width"], j["scr_taps"], j["scr_init"] = scr_width, scr_taps, scr_init
            at += Fosphor.rs_owned(Fosphor._rs_n_data(j)) + 8 * ((int(gap) + 7) // 8)
        return out

    @staticmethod
    def _rs_cap(jobs):
        return max([int(j["out_offset"]) + Fosphor.rs_owned(Fosphor._rs_n_data(j)) for j in jobs] + [0])

    def rs(self, d_in, jobs, n_bytes=None):
        """One record and the corrected data bytes per job, up to 4096 frames in one call (fosphor_amd_rs): the decoded bits of
        decode() or soft() taken as interleaved Reed-Solomon frames over GF(2^8), descrambled, every codeword corrected up to
        n_roots / 2 byte errors, the parity dropped, over bytes that are already in device memory.  d_in: a contiguous uint8
        device tensor (what decode() or soft() wrote) or a raw device pointer with n_bytes; jobs: an RS_JOB_DTYPE array (rs_jobs()
        makes one; out_offset is honoured, the owned bytes must not overlap).
        Returns (records, views): an RS_RECORD_DTYPE array copied from the device, in job order, and a list with one torch uint8
        view of n_data bytes per job into one device buffer."""
        import torch
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=self.RS_JOB_DTYPE)
        if n_bytes is None:
            if not hasattr(d_in, "numel"):
                raise ValueError("a raw device pointer needs n_bytes")
            if str(d_in.dtype) != "torch.uint8" or not d_in.is_contiguous():
                raise ValueError("d_in must be a contiguous uint8 tensor")
            n_bytes = d_in.numel()
        cap = self._rs_cap(jobs)
        # torch.empty: a fill would run on torch's stream, unordered against the pass on the instance's
        d_out = torch.empty(max(cap, 8) // 8, dtype=torch.int64, device="cuda").view(torch.uint8)
        d_rec = torch.empty(max(jobs.size, 1) * self.RS_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()			# the caller's bytes were written on torch's stream
        rv = self.L.fosphor_amd_rs(self.h, _ptr(d_in), int(n_bytes), jobs.ctypes.data, int(jobs.size), d_rec.data_ptr(),
                                   d_out.data_ptr(), cap)
        if rv:
            _fail("fosphor_amd_rs", rv, RuntimeError)
        records = d_rec.cpu().numpy().view(self.RS_RECORD_DTYPE)[:jobs.size].copy()
        return records, [d_out[int(j["out_offset"]):int(j["out_offset"]) + int(r["n_data"])] for j, r in zip(jobs, records)]

    @staticmethod
    def rs_host(data, jobs):
        """fosphor_amd_rs_host: the same records and bytes on the host, no GPU.  data: uint8.  Returns (records, views), the views
        uint8 arrays of n_data bytes into one buffer"""
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.RS_JOB_DTYPE)
        cap = Fosphor._rs_cap(jobs)
        out = np.zeros(max(cap, 8) // 8, np.uint64).view(np.uint8)
        records = np.zeros(max(jobs.size, 1), Fosphor.RS_RECORD_DTYPE)
        keep = data if data.size else np.zeros(8, np.uint8)
        rv = _lib.load().fosphor_amd_rs_host(keep.ctypes.data, int(data.size), jobs.ctypes.data, int(jobs.size),
                                             records.ctypes.data, out.ctypes.data, cap)
        if rv:
            _fail("fosphor_amd_rs_host", rv, ValueError)
        records = records[:jobs.size]
        return records, [out[int(j["out_offset"]):int(j["out_offset"]) + int(r["n_data"])] for j, r in zip(jobs, records)]

    @staticmethod
    def rs_encode(data, jobs, n_bytes=None):
        """fosphor_amd_rs_encode_host: the way back.  Job j takes its n_data bytes from data[out_offset ..), in the order rs()
        writes them, and its frame of depth * n_code bytes, parity added and scrambled as flagged, goes to frames[offset ..).
        Returns the frames buffer, uint8 [n_bytes] (the end of the last frame by default), zero where no frame lies"""
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        jobs = np.ascontiguousarray(np.atleast_1d(jobs), dtype=Fosphor.RS_JOB_DTYPE)
        if n_bytes is None:
            n_bytes = max([int(j["offset"]) + int(j["depth"]) * int(j["n_code"]) for j in jobs] + [0])
        frames = np.zeros(max(int(n_bytes), 1), np.uint8)
        keep = data if data.size else np.zeros(8, np.uint8)
        rv = _lib.load().fosphor_amd_rs_encode_host(keep.ctypes.data, int(data.size), jobs.ctypes.data, int(jobs.size),
                                                    frames.ctypes.data, int(n_bytes))
        if rv:
            _fail("fosphor_amd_rs_encode_host", rv, ValueError)
        return frames[:max(int(n_bytes), 0)]

    @staticmethod
    def rs_derive(records):
        """fosphor_amd_rs_derive per record: a list of dicts of RS_VALUES (ratios)"""
        L = _lib.load()
        records = np.ascontiguousarray(np.atleast_1d(records), dtype=Fosphor.RS_RECORD_DTYPE)
        out = []
        for r in records:
            v = _lib.RsValues()
            rv = L.fosphor_amd_rs_derive(r.tobytes(), C.byref(v))
            if rv:
                _fail("fosphor_amd_rs_derive", rv, ValueError)
            out.append({k: getattr(v, k) for k in Fosphor.RS_VALUES})
        return out

    def rs_stats(self):
        """fosphor_amd_rs_stats as a dict: calls, launches by kernel, codewords, clean and failed ones (RS_STATS)"""
        return self._stats(self.L.fosphor_amd_rs_stats, self.RS_STATS)

    @property
    def histo_scale(self):
        return self.buffers(False).histo_scale

    @property
    def histo_offset(self):
        return self.buffers(False).histo_offset

    # ---- kernel-level hooks -------------------------------------------------
    def fft_device(self, d_in, d_out, n_spectra):
        return self.L.fosphor_amd_fft(self.h, self._dev(d_in), _ptr(d_out), n_spectra)

    def bin_device(self, d_fft, d_bin, d_pwr, n):
        return self.L.fosphor_amd_bin(self.h, _ptr(d_fft), _ptr(d_bin), _ptr(d_pwr), n)

    # ---- measurement --------------------------------------------------------
    def profile(self, enable=True):
        """False/0: off; True/1: hipEvents around every kernel; 2: around K1 only."""
        self.L.fosphor_amd_profile(self.h, 2 if enable == 2 and enable is not True else (1 if enable else 0))

    def tune_placement(self, d_samples, n_batches, batch, max_tries=6):
        """fosphor_amd_tune_placement: (re-allocations made, slowest set's twin us before, after)."""
        b, a = C.c_float(), C.c_float()
        rv = self.L.fosphor_amd_tune_placement(self.h, _ptr(d_samples), int(n_batches), int(batch), int(max_tries), C.byref(b), C.byref(a))
        if rv < 0:
            raise RuntimeError("fosphor_amd_tune_placement -> %d" % rv)
        return rv, b.value, a.value

    def traffic_twin(self, d_samples, n_batches, batch, reps=20):
        """ms per launch of K1's memory traffic alone (include/fosphor_amd.h)"""
        ms = C.c_float()
        rv = self.L.fosphor_amd_traffic_twin(self.h, _ptr(d_samples), int(n_batches), int(batch), int(reps), C.byref(ms))
        if rv:
            raise RuntimeError("fosphor_amd_traffic_twin -> %d" % rv)
        return ms.value

    def set_overlap(self, enable):
        return self.L.fosphor_amd_set_overlap(self.h, 1 if enable else 0)

    def set_input_ordering(self, strict):
        return self.L.fosphor_amd_set_input_ordering(self.h, 1 if strict else 0)

    def wait_input(self):
        return self.L.fosphor_amd_wait_input(self.h)

    def exchange_time(self):
        """(ms summed over the exchanges recorded while profiling was on, how many); resets"""
        ms, n = C.c_float(), C.c_int()
        rv = self.L.fosphor_amd_exchange_time(self.h, C.byref(ms), C.byref(n))
        if rv:
            raise RuntimeError("fosphor_amd_exchange_time -> %d" % rv)
        return ms.value, n.value

    def share_stats(self):
        """fosphor_amd_share_stats: (FFT launches in the space-sharing form, in the full-chip form, work-groups of the shared form)"""
        a, b, c = C.c_longlong(), C.c_longlong(), C.c_int()
        rv = self.L.fosphor_amd_share_stats(self.h, C.byref(a), C.byref(b), C.byref(c))
        if rv:
            raise RuntimeError("fosphor_amd_share_stats -> %d" % rv)
        return a.value, b.value, c.value

    def launch_stats(self):
        """fosphor_amd_launch_stats: (FFT pieces launched by accumulate_device, chunk sums over 16-bit slabs, chunk reduces with
        32-bit counts) since the instance was made"""
        a, b, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
        rv = self.L.fosphor_amd_launch_stats(self.h, C.byref(a), C.byref(b), C.byref(c))
        if rv:
            raise RuntimeError("fosphor_amd_launch_stats -> %d" % rv)
        return a.value, b.value, c.value

    MERGE_FORMS = ("dense16", "dense16_long4", "dense16_long", "table32", "eval32", "sparse16", "sparse16_long", "table_in_memory",
                   "sparse_max_batches", "sparse_long_max_batches", "sparse_listed_rows")

    def merge_stats(self):
        """fosphor_amd_merge_stats as a dict: merge launches since the instance was made by form (MERGE_FORMS[:7]), how many of the
        long-batch ones read the rise/decay table from memory, the most batches one sparse launch of either kind merged, the rows the last sparse launch listed (-1: none yet; waits for it)"""
        return self._stats(self.L.fosphor_amd_merge_stats, self.MERGE_FORMS)

    def kernel_busy(self):
        """ms during which >= 1 kernel of each kind ran (call before kernel_times)"""
        ms = (C.c_float * 3)()
        rv = self.L.fosphor_amd_kernel_busy(self.h, C.byref(ms))
        if rv:
            raise RuntimeError("fosphor_amd_kernel_busy -> %d" % rv)
        return list(ms)

    def kernel_times(self):
        ms = (C.c_float * 3)()
        n = (C.c_int * 3)()
        rv = self.L.fosphor_amd_kernel_times(self.h, C.byref(ms), C.byref(n))
        if rv:
            raise RuntimeError("fosphor_amd_kernel_times -> %d" % rv)
        return list(ms), list(n)

    @property
    def stream(self):
        return self.L.fosphor_amd_stream(self.h)

    @property
    def stream2(self):
        return self.L.fosphor_amd_stream2(self.h)
