"""Host-side mirror of the reference's generators for the hot path.

ImageCompressorTop <- class ImageCompressorTop(...), ImageCompressorTop.scala:11-25 (same 11-argument
                      list, same order, same require()s); instead of a Decoupled `io` bundle driven one
                      pixel per simulated clock (ImageCompressorTopApp.scala:76-124) it exposes
                      process(): one fused HIP kernel launch per frame.
ImageProcessor     <- class ImageProcessor(p: ImageProcessorParams), ImageProcessor.scala:31-63.
Plan               <- thin RAII wrapper of csic_plan (include/csic.h).

Device memory and streams come from PyTorch (plumbing only): CUDA tensors are passed by data_ptr and
the launch goes to torch's current stream.  numpy inputs take csic_process_host (H2D + kernel + D2H).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Tuple

import numpy as np

from . import _native as N
from .container import (delta_host, delta_layout, mc_delta_host, mc_layout, mc_undelta_host, rows_host, rows_layout, unrows_host, pack_frame_host, rans_pack_host, rans_unpack_host,
                        rice_pack_host, rice_unpack_host, undelta_host, unpack_frame_host)
from .params import (ImageProcessorParams, PixelFormat, ProcessingStep, Rounding, Sampling, make_c_params)


def _is_torch_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


class View(NamedTuple):
    """A window of a decoded frame for Plan.decode_view_* (csic_view): the source rectangle starts at (x0, y0) and covers width *
    scale x height * scale decoded pixels; width and height count OUTPUT pixels; scale is 1, 2, 4, 8 or 16."""
    x0: int
    y0: int
    width: int
    height: int
    scale: int = 1


class Distortion:
    """The six sums of squared errors of one frame (csic_distortion_*; definition in include/csic.h), in the order
    R, G, B, Y, Cb, Cr, over `pixels` input pixels; mse / psnr per channel (index or name), psnr_rgb over R, G and B
    together.  PSNR is +inf at zero error."""

    CHANNELS = ("R", "G", "B", "Y", "Cb", "Cr")

    def __init__(self, sse, pixels: int):
        self.sse = tuple(int(v) for v in sse)
        if len(self.sse) != N.DIST_CHANNELS:
            raise ValueError(f"need {N.DIST_CHANNELS} sums (R, G, B, Y, Cb, Cr), got {len(self.sse)}")
        self.pixels = int(pixels)

    def _index(self, ch) -> int:
        return self.CHANNELS.index(ch) if isinstance(ch, str) else int(ch)

    def mse(self, ch) -> float:
        return self.sse[self._index(ch)] / self.pixels

    def psnr(self, ch) -> float:
        e = self.sse[self._index(ch)]
        return math.inf if e == 0 else 10.0 * math.log10(255.0 * 255.0 * self.pixels / e)

    @property
    def psnr_rgb(self) -> float:
        e = self.sse[0] + self.sse[1] + self.sse[2]
        return math.inf if e == 0 else 10.0 * math.log10(255.0 * 255.0 * 3 * self.pixels / e)

    def __eq__(self, other) -> bool:
        return isinstance(other, Distortion) and (self.sse, self.pixels) == (other.sse, other.pixels)

    def __repr__(self) -> str:
        return f"Distortion(sse={self.sse}, pixels={self.pixels})"


class Ssim:
    """The six sums of the 8 x 8 block SSIM of one frame (csic_ssim_*; definition in include/csic.h), in the order
    R, G, B, Y, Cb, Cr: each the sum of the windows' 16.16 fixed-point quotients over `windows` windows.  mean(ch) is the
    channel's mean SSIM (index or name), mean_rgb the mean of the R, G and B means; 1.0 exactly for an output equal to the input."""

    CHANNELS = Distortion.CHANNELS

    def __init__(self, sums, windows: int):
        self.sums = tuple(int(v) for v in sums)
        if len(self.sums) != N.DIST_CHANNELS:
            raise ValueError(f"need {N.DIST_CHANNELS} sums (R, G, B, Y, Cb, Cr), got {len(self.sums)}")
        self.windows = int(windows)

    def _index(self, ch) -> int:
        return self.CHANNELS.index(ch) if isinstance(ch, str) else int(ch)

    def mean(self, ch) -> float:
        return self.sums[self._index(ch)] / (N.SSIM_ONE * self.windows)

    @property
    def mean_rgb(self) -> float:
        return (self.mean(0) + self.mean(1) + self.mean(2)) / 3.0

    def __eq__(self, other) -> bool:
        return isinstance(other, Ssim) and (self.sums, self.windows) == (other.sums, other.windows)

    def __repr__(self) -> str:
        return f"Ssim(sums={self.sums}, windows={self.windows})"


class CodeStats:
    """The histograms of one compressed frame (csic_code_stats_*; definition in include/csic.h): hist[kind][plane] is a uint64
    array of 256 counts, kind 0 = the sample codes, 1 = their left-predicted residuals, planes Y, Cb, Cr (index or name) with
    bits[plane] bits per code and samples[plane] samples.  entropy(kind, plane) is the zero-order entropy in bits per sample,
    bits_per_pixel(kind) / ideal_bytes(kind) what an ideal order-0 coder of that kind spends on the frame per input pixel / in
    bytes; kind "best" takes per plane the cheapest of raw, codes and residuals.  All in double precision from the counts."""

    KINDS = ("codes", "residuals")
    PLANES = ("Y", "Cb", "Cr")

    def __init__(self, hist, bits, pixels: int):
        self.hist = np.array(hist, dtype=np.uint64).reshape(N.STATS_KINDS, N.STATS_PLANES, N.STATS_BINS)
        self.bits = tuple(int(v) for v in bits)
        if len(self.bits) != N.STATS_PLANES:
            raise ValueError(f"need {N.STATS_PLANES} bit widths (Y, Cb, Cr), got {len(self.bits)}")
        self.pixels = int(pixels)
        self.samples = tuple(int(self.hist[0, p].sum()) for p in range(N.STATS_PLANES))

    def _kind(self, kind) -> int:
        return self.KINDS.index(kind) if isinstance(kind, str) else int(kind)

    def _plane(self, plane) -> int:
        return self.PLANES.index(plane) if isinstance(plane, str) else int(plane)

    def entropy(self, kind, plane) -> float:
        h = self.hist[self._kind(kind), self._plane(plane)].astype(np.float64)
        total = h.sum()
        if total == 0:
            return 0.0
        p = h[h > 0] / total
        return max(0.0, float(-(p * np.log2(p)).sum()))

    def _plane_bits(self, kind, p: int) -> float:
        """Bits plane p takes under `kind` (0, 1 or "best")."""
        if kind == "best":
            return self.samples[p] * min(float(self.bits[p]), self.entropy(0, p), self.entropy(1, p))
        return self.samples[p] * self.entropy(kind, p)

    def total_bits(self, kind) -> float:
        return sum(self._plane_bits(kind, p) for p in range(N.STATS_PLANES))

    def bits_per_pixel(self, kind) -> float:
        return self.total_bits(kind) / self.pixels

    def ideal_bytes(self, kind) -> int:
        return int(math.ceil(self.total_bits(kind) / 8.0))

    @property
    def raw_bits_per_pixel(self) -> float:
        return sum(n * q for n, q in zip(self.samples, self.bits)) / self.pixels

    def __eq__(self, other) -> bool:
        return isinstance(other, CodeStats) and (self.bits, self.pixels) == (other.bits, other.pixels) \
            and np.array_equal(self.hist, other.hist)

    __hash__ = None

    def __repr__(self) -> str:
        return (f"CodeStats(samples={self.samples}, bits={self.bits}, pixels={self.pixels}, raw={self.raw_bits_per_pixel:.4f}, "
                f"H0={self.bits_per_pixel(0):.4f}, H1={self.bits_per_pixel(1):.4f}, best={self.bits_per_pixel('best'):.4f} bits/px)")


class QSweep:
    """The quantiser sweep of one frame, or of several frames together (csic_qsweep_*; definition in include/csic.h): sse[p][q - 1]
    is the sum of squared errors of plane p (Y, Cb, Cr: index or name) at bit width q and hist[p][q - 1] the 256 counts of the
    left-predicted residuals of that plane at that width, both uint64 and exact; with several frames the leading axis is the
    frame.  psnr(p, q) is the plane's PSNR at width q over all frames; est_bytes(bits, coding) and rank(coding, weights, max_bits)
    are csic_qsweep_rank's figures."""

    PLANES = ("Y", "Cb", "Cr")
    CODINGS = {"raw": N.CODING_RAW, "groups": N.CODING_GROUPS, "rice": N.CODING_RICE, "rans": N.CODING_RANS}

    def __init__(self, result, c_params: N.CsicParams):
        raw = np.ascontiguousarray(result).view(np.uint64).reshape(-1, C.sizeof(N.CsicQsweepResult) // 8)
        self._raw = raw
        self.nframes = raw.shape[0]
        nsse = N.STATS_PLANES * N.QSWEEP_WIDTHS
        self.sse = raw[:, :nsse].reshape(-1, N.STATS_PLANES, N.QSWEEP_WIDTHS)
        self.hist = raw[:, nsse:].reshape(-1, N.STATS_PLANES, N.QSWEEP_WIDTHS, N.STATS_BINS)
        if self.nframes == 1:
            self.sse, self.hist = self.sse[0], self.hist[0]
        self.c_params = c_params
        self.pixels = c_params.width * c_params.height

    def _plane(self, plane) -> int:
        return self.PLANES.index(plane) if isinstance(plane, str) else int(plane)

    @classmethod
    def _coding(cls, coding) -> int:
        return cls.CODINGS[coding] if isinstance(coding, str) else int(coding)

    def psnr(self, plane, q: int) -> float:
        e = int(self._raw[:, self._plane(plane) * N.QSWEEP_WIDTHS + int(q) - 1].sum())
        return math.inf if e == 0 else 10.0 * math.log10(255.0 * 255.0 * self.pixels * self.nframes / e)

    def rank(self, coding="rans", weights=(1, 1, 1), max_bits=(8, 8, 8)):
        """Every (y, cb, cr) with 1 <= q_p <= max_bits[p] in ascending order of (distortion, est_bytes, y, cb, cr): a list of
        (distortion, est_bytes, (y, cb, cr)) (csic_qsweep_rank)."""
        if any(not 0 <= int(v) <= 255 for v in tuple(weights) + tuple(max_bits)) or len(weights) != 3 or len(max_bits) != 3:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: weights and max_bits are three values in 0..255")
        w = (C.c_uint8 * 3)(*[int(v) for v in weights])
        mb = (C.c_uint8 * 3)(*[int(v) for v in max_bits])
        out = (N.CsicQsweepCandidate * N.QSWEEP_MAX_CANDIDATES)()
        n = C.c_int32(N.QSWEEP_MAX_CANDIDATES)
        N.check(N.lib().csic_qsweep_rank(C.byref(self.c_params), self._raw.ctypes.data_as(C.c_void_p), self.nframes, self._coding(coding),
                                         w, mb, out, C.byref(n)))
        return [(c.distortion, c.est_bytes, (c.y_bits, c.cb_bits, c.cr_bits)) for c in out[:n.value]]

    def est_bytes(self, bits, coding="rans") -> int:
        """The size estimate of the bit set `bits` = (y, cb, cr) under `coding`; exact for "raw"."""
        bits = tuple(int(b) for b in bits)
        for _, est, b in self.rank(coding, (1, 1, 1), bits):
            if b == bits:
                return est
        raise AssertionError("csic_qsweep_rank lists every bit set up to max_bits")

    def __repr__(self) -> str:
        return f"QSweep(nframes={self.nframes}, pixels={self.pixels}, psnr_y8={self.psnr(0, 8):.2f}, psnr_y1={self.psnr(0, 1):.2f})"


class Plan:
    """One validated parameter set bound to one HIP device (csic_plan_create / csic_plan_destroy)."""

    def __init__(self, c_params: N.CsicParams, device: int = 0):
        self._h = C.c_void_p()
        self.c_params = c_params
        self.device = int(device)
        N.check(N.lib().csic_plan_create(C.byref(c_params), self.device, C.byref(self._h)))
        wo, ho = C.c_int32(), C.c_int32()
        N.check(N.lib().csic_out_dims(C.byref(c_params), C.byref(wo), C.byref(ho)))
        self.width, self.height = c_params.width, c_params.height
        self.out_width, self.out_height = wo.value, ho.value

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            N.lib().csic_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- introspection ----------------------------------------------------------------------------
    @property
    def kernel_name(self) -> str:
        return N.lib().csic_plan_kernel_name(self._h).decode()

    @property
    def algorithmic_bytes(self) -> int:
        b = C.c_int64()
        N.check(N.lib().csic_algorithmic_bytes(C.byref(self.c_params), C.byref(b)))
        return b.value

    def tune(self, knob: int, value: int) -> None:
        N.check(N.lib().csic_plan_tune(self._h, knob, value))

    @property
    def planar(self) -> bool:
        return self.c_params.out_format == N.FMT_PLANAR

    @property
    def planar_layout(self) -> N.CsicPlanarLayout:
        """csic_planar_layout of these parameters (whatever the plan's out_format is)."""
        lay = N.CsicPlanarLayout()
        N.check(N.lib().csic_planar_layout_of(C.byref(self.c_params), C.byref(lay)))
        return lay

    @property
    def planar_bits(self) -> bool:
        return self.c_params.out_format == N.FMT_PLANAR_BITS

    @property
    def planar_bits_layout(self) -> N.CsicPlanarBitsLayout:
        """csic_planar_bits_layout of these parameters (whatever the plan's out_format is)."""
        lay = N.CsicPlanarBitsLayout()
        N.check(N.lib().csic_planar_bits_layout_of(C.byref(self.c_params), C.byref(lay)))
        return lay

    @property
    def frame_bytes(self) -> int:
        """Bytes of one output frame buffer of a planar (PLANAR / PLANAR_BITS) plan."""
        return self.planar_bits_layout.frame_bytes if self.planar_bits else self.planar_layout.frame_bytes

    @property
    def preferred_pitch(self) -> Tuple[int, int]:
        """(in_pitch_px, out_pitch_px) at which a caller that owns its surfaces should lay frames out (csic_plan_preferred_pitch)."""
        ip, op = C.c_int32(), C.c_int32()
        N.check(N.lib().csic_plan_preferred_pitch(self._h, C.byref(ip), C.byref(op)))
        return ip.value, op.value

    # -- distortion (csic_distortion_*) ----------------------------------------------------------
    @property
    def distortion_kernel_name(self) -> str:
        return N.lib().csic_distortion_kernel_name(self._h).decode()

    def distortion_workspace_bytes(self, nframes: int = 1) -> int:
        b = C.c_size_t()
        N.check(N.lib().csic_distortion_workspace_bytes(self._h, int(nframes), C.byref(b)))
        return b.value

    def distortion_device(self, d_in, nframes: int = 1, d_sse=None):
        """d_in: contiguous 4-byte CUDA tensor of nframes * W * H input pixels.  Returns an int64 tensor (nframes, 6) on the
        device: the sums R, G, B, Y, Cb, Cr of each frame (never above 2^63).  Asynchronous on torch's current stream; the plan
        keeps its workspace between calls (allocate it with a first call before capturing the call into a graph)."""
        import torch
        if not d_in.is_cuda or d_in.element_size() != 4 or not d_in.is_contiguous():
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_in must be a contiguous 4-byte CUDA tensor")
        if d_in.device.index != self.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: tensor is on a different device than the plan")
        if d_in.numel() != nframes * self.width * self.height:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: expected {nframes * self.width * self.height} input pixels, got {d_in.numel()}")
        need = self.distortion_workspace_bytes(nframes)
        ws = getattr(self, "_dist_ws", None)
        if ws is None or ws.numel() * 8 < need or ws.device != d_in.device:
            ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=d_in.device)
            self._dist_ws = ws
        if d_sse is None:
            d_sse = torch.empty((nframes, N.DIST_CHANNELS), dtype=torch.int64, device=d_in.device)
        elif d_sse.numel() != nframes * N.DIST_CHANNELS or d_sse.element_size() != 8 or not d_sse.is_contiguous():
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_sse must be a contiguous 8-byte tensor of nframes * 6")
        N.check(N.lib().csic_distortion_device(self._h, C.c_void_p(d_in.data_ptr()), int(nframes), C.c_void_p(d_sse.data_ptr()),
                                               C.c_void_p(ws.data_ptr()), ws.numel() * 8, self._stream()))
        return d_sse

    def distortion_host(self, frames: np.ndarray, nframes: int = 1) -> np.ndarray:
        """csic_distortion_host: nframes * W * H host pixels -> uint64 array (nframes, 6)."""
        a = np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1)
        sse = np.zeros((nframes, N.DIST_CHANNELS), dtype=np.uint64)
        N.check(N.lib().csic_distortion_host(self._h, a.ctypes.data_as(C.c_void_p), a.size, int(nframes),
                                             sse.ctypes.data_as(C.POINTER(C.c_uint64))))
        return sse

    def distortion(self, frames):
        """One frame ((H, W), or flat W * H) -> Distortion; a stack (n, H, W) -> list of Distortion.  numpy input goes through
        csic_distortion_host, a CUDA tensor through distortion_device (synchronised here)."""
        px = self.width * self.height
        if _is_torch_tensor(frames):
            n = frames.numel() // px if px else 0
            sse = self.distortion_device(frames.contiguous(), n).cpu().numpy()
            single = frames.dim() != 3
        else:
            a = np.asarray(frames)
            n = a.size // px if px else 0
            sse = self.distortion_host(a, n)
            single = a.ndim != 3
        out = [Distortion(row, px) for row in sse]
        return out[0] if single and n == 1 else out

    # -- structural similarity (csic_ssim_*) -----------------------------------------------------
    @property
    def ssim_kernel_name(self) -> str:
        return N.lib().csic_ssim_kernel_name(self._h).decode()

    @property
    def ssim_windows(self) -> Tuple[int, int]:
        """(rows, columns) of 8 x 8 windows in a frame."""
        return self.height // N.SSIM_WINDOW, self.width // N.SSIM_WINDOW

    def ssim_workspace_bytes(self, nframes: int = 1) -> int:
        b = C.c_size_t()
        N.check(N.lib().csic_ssim_workspace_bytes(self._h, int(nframes), C.byref(b)))
        return b.value

    def ssim_device(self, d_in, nframes: int = 1, want_map: bool = False):
        """d_in: contiguous 4-byte CUDA tensor of nframes * W * H input pixels.  Returns an int64 tensor (nframes, 6) on the
        device: the sums of the windows' quotients for R, G, B, Y, Cb, Cr of each frame; with want_map, (sums, map), the map an
        int32 tensor (nframes, 6, H / 8, W / 8) of the quotients themselves.  Asynchronous on torch's current stream; the plan
        keeps its workspace between calls (allocate it with a first call before capturing the call into a graph)."""
        import torch
        if not d_in.is_cuda or d_in.element_size() != 4 or not d_in.is_contiguous():
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_in must be a contiguous 4-byte CUDA tensor")
        if d_in.device.index != self.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: tensor is on a different device than the plan")
        if d_in.numel() != nframes * self.width * self.height:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: expected {nframes * self.width * self.height} input pixels, got {d_in.numel()}")
        need = self.ssim_workspace_bytes(nframes)
        ws = getattr(self, "_ssim_ws", None)
        if ws is None or ws.numel() * 8 < need or ws.device != d_in.device:
            ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=d_in.device)
            self._ssim_ws = ws
        d_ssim = torch.empty((nframes, N.DIST_CHANNELS), dtype=torch.int64, device=d_in.device)
        d_map = torch.empty((nframes, N.DIST_CHANNELS) + self.ssim_windows, dtype=torch.int32, device=d_in.device) if want_map else None
        N.check(N.lib().csic_ssim_device(self._h, C.c_void_p(d_in.data_ptr()), int(nframes), C.c_void_p(d_ssim.data_ptr()),
                                         C.c_void_p(d_map.data_ptr()) if want_map else None, C.c_void_p(ws.data_ptr()),
                                         ws.numel() * 8, self._stream()))
        return (d_ssim, d_map) if want_map else d_ssim

    def ssim_host(self, frames: np.ndarray, nframes: int = 1, want_map: bool = False):
        """csic_ssim_host: nframes * W * H host pixels -> int64 array (nframes, 6); with want_map, (sums, map), the map an int32
        array (nframes, 6, H / 8, W / 8)."""
        a = np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1)
        sums = np.zeros((nframes, N.DIST_CHANNELS), dtype=np.int64)
        smap = np.zeros((nframes, N.DIST_CHANNELS) + self.ssim_windows, dtype=np.int32) if want_map else None
        N.check(N.lib().csic_ssim_host(self._h, a.ctypes.data_as(C.c_void_p), a.size, int(nframes),
                                       sums.ctypes.data_as(C.POINTER(C.c_int64)), smap.ctypes.data_as(C.c_void_p) if want_map else None))
        return (sums, smap) if want_map else sums

    def ssim(self, frames):
        """One frame ((H, W), or flat W * H) -> Ssim; a stack (n, H, W) -> list of Ssim.  numpy input goes through csic_ssim_host,
        a CUDA tensor through ssim_device (synchronised here)."""
        px = self.width * self.height
        if _is_torch_tensor(frames):
            n = frames.numel() // px if px else 0
            sums = self.ssim_device(frames.contiguous(), n).cpu().numpy()
            single = frames.dim() != 3
        else:
            a = np.asarray(frames)
            n = a.size // px if px else 0
            sums = self.ssim_host(a, n)
            single = a.ndim != 3
        wy, wx = self.ssim_windows
        out = [Ssim(row, wy * wx) for row in sums]
        return out[0] if single and n == 1 else out

    # -- quantiser sweep (csic_qsweep_*) -----------------------------------------------------------
    @property
    def qsweep_kernel_name(self) -> str:
        return N.lib().csic_qsweep_kernel_name(self._h).decode()

    @property
    def qsweep_block_samples(self) -> int:
        """Consecutive samples of a plane that one block of the histogram kernel counts (csic_qsweep_block_samples)."""
        b = C.c_int64()
        N.check(N.lib().csic_qsweep_block_samples(self._h, C.byref(b)))
        return b.value

    def qsweep_workspace_bytes(self, nframes: int = 1) -> int:
        b = C.c_size_t()
        N.check(N.lib().csic_qsweep_workspace_bytes(self._h, int(nframes), C.byref(b)))
        return b.value

    def _qsweep_result(self, nframes: int, device, d_result):
        import torch
        words = C.sizeof(N.CsicQsweepResult) // 8
        if d_result is None:
            return torch.empty((nframes, words), dtype=torch.int64, device=device)
        if d_result.numel() != nframes * words or d_result.element_size() != 8 or not d_result.is_contiguous():
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: d_result must be a contiguous 8-byte tensor of nframes * {words}")
        return d_result

    def qsweep_device(self, d_in, nframes: int = 1, d_result=None):
        """d_in: contiguous 4-byte CUDA tensor of nframes * W * H input pixels.  Returns an int64 tensor (nframes, 6168) on the
        device: each frame's csic_qsweep_result as 64-bit words (QSweep reads it).  Asynchronous on torch's current stream; the plan
        keeps its workspace between calls (allocate it with a first call before capturing the call into a graph)."""
        import torch
        if not d_in.is_cuda or d_in.element_size() != 4 or not d_in.is_contiguous():
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_in must be a contiguous 4-byte CUDA tensor")
        if d_in.device.index != self.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: tensor is on a different device than the plan")
        if d_in.numel() != nframes * self.width * self.height:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: expected {nframes * self.width * self.height} input pixels, got {d_in.numel()}")
        need = self.qsweep_workspace_bytes(nframes)
        ws = getattr(self, "_qsweep_ws", None)
        if ws is None or ws.numel() < need or ws.device != d_in.device:
            ws = torch.empty(need, dtype=torch.uint8, device=d_in.device)
            self._qsweep_ws = ws
        d_result = self._qsweep_result(nframes, d_in.device, d_result)
        N.check(N.lib().csic_qsweep_device(self._h, C.c_void_p(d_in.data_ptr()), int(nframes), C.c_void_p(d_result.data_ptr()),
                                           C.c_void_p(ws.data_ptr()), ws.numel(), self._stream()))
        return d_result

    def qsweep_hist_device(self, d_planar, nframes: int = 1, d_result=None):
        """d_planar: contiguous CUDA tensor of nframes CSIC_FMT_PLANAR frame buffers.  Fills `hist` of d_result (as qsweep_device
        returns it; a new one is zeroed first) and leaves its `sse` as it was (csic_qsweep_hist_device)."""
        import torch
        if not d_planar.is_cuda or not d_planar.is_contiguous() or d_planar.numel() * d_planar.element_size() != nframes * self.planar_layout.frame_bytes:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_planar must be a contiguous CUDA tensor of nframes PLANAR frames")
        if d_planar.device.index != self.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: tensor is on a different device than the plan")
        if d_result is None:
            d_result = torch.zeros((nframes, C.sizeof(N.CsicQsweepResult) // 8), dtype=torch.int64, device=d_planar.device)
        d_result = self._qsweep_result(nframes, d_planar.device, d_result)
        N.check(N.lib().csic_qsweep_hist_device(self._h, C.c_void_p(d_planar.data_ptr()), int(nframes), C.c_void_p(d_result.data_ptr()),
                                                self._stream()))
        return d_result

    def qsweep_host(self, frames: np.ndarray, nframes: int = 1) -> np.ndarray:
        """csic_qsweep_host: nframes * W * H host pixels -> uint64 array (nframes, 6168)."""
        a = np.ascontiguousarray(frames, dtype=np.uint32).reshape(-1)
        res = np.zeros((nframes, C.sizeof(N.CsicQsweepResult) // 8), dtype=np.uint64)
        N.check(N.lib().csic_qsweep_host(self._h, a.ctypes.data_as(C.c_void_p), a.size, int(nframes), res.ctypes.data_as(C.c_void_p)))
        return res

    def qsweep(self, frames) -> QSweep:
        """One frame ((H, W), or flat W * H) or a stack (n, H, W) -> QSweep.  numpy input goes through csic_qsweep_host, a CUDA
        tensor through qsweep_device (synchronised here)."""
        px = self.width * self.height
        if _is_torch_tensor(frames):
            n = frames.numel() // px if px else 0
            res = self.qsweep_device(frames.contiguous().reshape(-1), n).cpu().numpy()
        else:
            a = np.asarray(frames)
            n = a.size // px if px else 0
            res = self.qsweep_host(a, n)
        return QSweep(res, self.c_params)

    # -- code statistics (csic_code_stats_*) ------------------------------------------------------
    def _stats_format(self, src_format) -> int:
        src_format = self.c_params.out_format if src_format is None else int(src_format)
        if src_format not in (N.FMT_PLANAR, N.FMT_PLANAR_BITS):
            raise N.IllegalArgumentException(N.EINVAL_FORMAT, f"requirement failed: code statistics read PLANAR or PLANAR_BITS frames, not format {src_format}")
        return src_format

    def code_stats_kernel_name(self, src_format=None) -> str:
        return N.lib().csic_code_stats_kernel_name(self._h, self._stats_format(src_format)).decode()

    def code_stats_block_samples(self, src_format=None) -> int:
        """Consecutive samples of a plane that one block counts (csic_code_stats_block_samples)."""
        b = C.c_int64()
        N.check(N.lib().csic_code_stats_block_samples(self._h, self._stats_format(src_format), C.byref(b)))
        return b.value

    def code_stats_device(self, d_src, src_format=None, nframes: int = 1):
        """d_src: contiguous CUDA tensor of nframes PLANAR / PLANAR_BITS frame buffers (None = the plan's own out_format).  Returns
        an int64 tensor (nframes, 2, 3, 256) on the device: the counts [kind][plane][bin] of each frame (never above 2^63).
        Asynchronous on torch's current stream; no workspace."""
        import torch
        src_format = self._stats_format(src_format)
        if not d_src.is_cuda or not d_src.is_contiguous() or d_src.numel() * d_src.element_size() != nframes * self._decode_src_bytes(src_format):
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_src must be a contiguous CUDA tensor of nframes source frames")
        if d_src.device.index != self.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: tensor is on a different device than the plan")
        d_hist = torch.empty((nframes, N.STATS_KINDS, N.STATS_PLANES, N.STATS_BINS), dtype=torch.int64, device=d_src.device)
        N.check(N.lib().csic_code_stats_device(self._h, C.c_void_p(d_src.data_ptr()), src_format, int(nframes),
                                               C.c_void_p(d_hist.data_ptr()), self._stream()))
        return d_hist

    def code_stats_host(self, buf, src_format=None, nframes: int = 1) -> np.ndarray:
        """csic_code_stats_host: nframes frame buffers in host memory -> uint64 array (nframes, 2, 3, 256)."""
        src_format = self._stats_format(src_format)
        a = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
        hist = np.zeros((nframes, N.STATS_KINDS, N.STATS_PLANES, N.STATS_BINS), dtype=np.uint64)
        N.check(N.lib().csic_code_stats_host(self._h, a.ctypes.data_as(C.c_void_p), a.size, src_format, int(nframes),
                                             hist.ctypes.data_as(C.c_void_p)))
        return hist

    def code_stats(self, src, src_format=None, nframes: int = 1):
        """One compressed frame -> CodeStats; nframes > 1 -> a list of them.  Host bytes go through csic_code_stats_host, a CUDA
        tensor through code_stats_device (synchronised here)."""
        if _is_torch_tensor(src):
            hist = self.code_stats_device(src.contiguous(), src_format, nframes).cpu().numpy().view(np.uint64)
        else:
            hist = self.code_stats_host(src, src_format, nframes)
        bits = (self.c_params.y_bits, self.c_params.cb_bits, self.c_params.cr_bits)
        out = [CodeStats(h, bits, self.width * self.height) for h in hist]
        return out[0] if nframes == 1 else out

    # -- lossless group coding of PLANAR_BITS frames (csic_pack_*) -------------------------------------
    @property
    def pack_layout(self) -> N.CsicPackLayout:
        """csic_pack_layout of these parameters: groups, section offsets, fixed_bytes, bound_bytes."""
        lay = N.CsicPackLayout()
        N.check(N.lib().csic_pack_layout_of(C.byref(self.c_params), C.byref(lay)))
        return lay

    @property
    def pack_kernel_name(self) -> str:
        return N.lib().csic_pack_kernel_name(self._h).decode()

    def pack_workspace_bytes(self, nframes: int = 1) -> int:
        b = C.c_size_t()
        N.check(N.lib().csic_pack_workspace_bytes(self._h, int(nframes), C.byref(b)))
        return b.value

    def _pack_check(self, t, nbytes: int, what: str) -> None:
        if not t.is_cuda or not t.is_contiguous() or t.numel() * t.element_size() != nbytes:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: {what} must be a contiguous CUDA tensor of {nbytes} bytes")
        if t.device.index != self.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: tensor is on a different device than the plan")

    def _pack_device(self, d_bits, nframes, d_coded, bound, workspace_bytes, pack):
        """pack_device / rice_pack_device: `bound`, `workspace_bytes` and `pack` are the coding's bound_bytes, *_workspace_bytes method
        and entry point."""
        import torch
        self._pack_check(d_bits, nframes * self.planar_bits_layout.frame_bytes, "d_bits")
        if d_coded is None:
            d_coded = torch.empty((nframes, bound), dtype=torch.uint8, device=d_bits.device)
        else:
            self._pack_check(d_coded, nframes * bound, "d_coded")
        sizes = torch.empty((nframes,), dtype=torch.int64, device=d_bits.device)
        wsb = workspace_bytes(nframes)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=d_bits.device)
        N.check(pack(self._h, C.c_void_p(d_bits.data_ptr()), int(nframes), C.c_void_p(d_coded.data_ptr()), C.c_void_p(sizes.data_ptr()),
                     C.c_void_p(ws.data_ptr()), wsb, self._stream()))
        return d_coded, sizes

    def _unpack_device(self, d_coded, nframes, d_bits, bound, workspace_bytes, unpack):
        """unpack_device / rice_unpack_device, as _pack_device; workspace_bytes is None for an entry point that takes no workspace."""
        import torch
        fb = self.planar_bits_layout.frame_bytes
        self._pack_check(d_coded, nframes * bound, "d_coded")
        if d_bits is None:
            d_bits = torch.empty((nframes, fb) if nframes > 1 else (fb,), dtype=torch.uint8, device=d_coded.device)
        else:
            self._pack_check(d_bits, nframes * fb, "d_bits")
        ws_args = ()
        if workspace_bytes is not None:
            wsb = workspace_bytes(nframes)
            ws = torch.empty((wsb,), dtype=torch.uint8, device=d_coded.device)
            ws_args = (C.c_void_p(ws.data_ptr()), wsb)
        N.check(unpack(self._h, C.c_void_p(d_coded.data_ptr()), int(nframes), C.c_void_p(d_bits.data_ptr()), *ws_args, self._stream()))
        return d_bits

    def pack_device(self, d_bits, nframes: int = 1, d_coded=None):
        """d_bits: nframes PLANAR_BITS frame buffers on the device (frame_bytes each).  Returns (coded, sizes): a uint8 tensor
        (nframes, bound_bytes) whose row k holds frame k's coded bytes in [0, sizes[k]) -- the rest of a row is not written -- and an
        int64 tensor (nframes,) of the coded sizes.  Asynchronous on torch's current stream."""
        return self._pack_device(d_bits, nframes, d_coded, self.pack_layout.bound_bytes, self.pack_workspace_bytes, N.lib().csic_pack_device)

    def unpack_device(self, d_coded, nframes: int = 1, d_bits=None):
        """The inverse of pack_device: d_coded holds nframes coded frames bound_bytes apart.  Returns the PLANAR_BITS frame buffers,
        a uint8 tensor (nframes, frame_bytes) (one frame: (frame_bytes,)); only their payload ranges are written.  The device does
        not validate: check untrusted bytes with unpack() first."""
        return self._unpack_device(d_coded, nframes, d_bits, self.pack_layout.bound_bytes, self.pack_workspace_bytes, N.lib().csic_unpack_device)

    def pack(self, bits_frame) -> np.ndarray:
        """csic_pack_host: one PLANAR_BITS frame buffer in host memory -> its coded bytes (uint8 array).  Needs no GPU."""
        return pack_frame_host(self.c_params, bits_frame)

    def unpack(self, coded, out=None) -> np.ndarray:
        """csic_unpack_host: coded bytes -> a PLANAR_BITS frame buffer (zero outside the payload ranges unless `out` is given)."""
        return unpack_frame_host(self.c_params, coded, out)

    # -- lossless Rice coding of PLANAR_BITS frames (csic_rice_*) ---------------------------------------
    @property
    def rice_layout(self) -> N.CsicRiceLayout:
        """csic_rice_layout of these parameters: groups, blocks, section offsets, fixed_bytes, bound_bytes."""
        lay = N.CsicRiceLayout()
        N.check(N.lib().csic_rice_layout_of(C.byref(self.c_params), C.byref(lay)))
        return lay

    @property
    def rice_kernel_name(self) -> str:
        return N.lib().csic_rice_kernel_name(self._h).decode()

    def rice_workspace_bytes(self, nframes: int = 1) -> int:
        b = C.c_size_t()
        N.check(N.lib().csic_rice_workspace_bytes(self._h, int(nframes), C.byref(b)))
        return b.value

    def rice_pack_device(self, d_bits, nframes: int = 1, d_coded=None):
        """As pack_device, in the Rice coding: returns (coded, sizes), a uint8 tensor (nframes, rice_layout.bound_bytes) whose row k
        holds frame k's coded bytes in [0, sizes[k]), and an int64 tensor of the sizes.  Asynchronous on torch's current stream."""
        return self._pack_device(d_bits, nframes, d_coded, self.rice_layout.bound_bytes, self.rice_workspace_bytes, N.lib().csic_rice_pack_device)

    def rice_unpack_device(self, d_coded, nframes: int = 1, d_bits=None):
        """The inverse of rice_pack_device, one pass without a workspace.  The device does not validate: check untrusted bytes with
        rice_unpack() first."""
        return self._unpack_device(d_coded, nframes, d_bits, self.rice_layout.bound_bytes, None, N.lib().csic_rice_unpack_device)

    def rice_pack(self, bits_frame) -> np.ndarray:
        """csic_rice_pack_host: one PLANAR_BITS frame buffer in host memory -> its Rice-coded bytes.  Needs no GPU."""
        return rice_pack_host(self.c_params, bits_frame)

    def rice_unpack(self, coded, out=None) -> np.ndarray:
        """csic_rice_unpack_host: Rice-coded bytes -> a PLANAR_BITS frame buffer."""
        return rice_unpack_host(self.c_params, coded, out)

    # -- lossless rANS coding of PLANAR_BITS frames (csic_rans_*) ---------------------------------------
    @property
    def rans_layout(self) -> N.CsicRansLayout:
        """csic_rans_layout of these parameters: groups, blocks, section offsets, fixed_bytes, bound_bytes."""
        lay = N.CsicRansLayout()
        N.check(N.lib().csic_rans_layout_of(C.byref(self.c_params), C.byref(lay)))
        return lay

    @property
    def rans_kernel_name(self) -> str:
        return N.lib().csic_rans_kernel_name(self._h).decode()

    def rans_workspace_bytes(self, nframes: int = 1) -> int:
        b = C.c_size_t()
        N.check(N.lib().csic_rans_workspace_bytes(self._h, int(nframes), C.byref(b)))
        return b.value

    def rans_pack_device(self, d_bits, nframes: int = 1, d_coded=None):
        """As pack_device, in the rANS coding: returns (coded, sizes), a uint8 tensor (nframes, rans_layout.bound_bytes) whose row k
        holds frame k's coded bytes in [0, sizes[k]), and an int64 tensor of the sizes.  Asynchronous on torch's current stream."""
        return self._pack_device(d_bits, nframes, d_coded, self.rans_layout.bound_bytes, self.rans_workspace_bytes, N.lib().csic_rans_pack_device)

    def rans_unpack_device(self, d_coded, nframes: int = 1, d_bits=None):
        """The inverse of rans_pack_device, one pass without a workspace.  The device does not validate: check untrusted bytes with
        rans_unpack() first."""
        return self._unpack_device(d_coded, nframes, d_bits, self.rans_layout.bound_bytes, None, N.lib().csic_rans_unpack_device)

    def rans_pack(self, bits_frame) -> np.ndarray:
        """csic_rans_pack_host: one PLANAR_BITS frame buffer in host memory -> its rANS-coded bytes.  Needs no GPU."""
        return rans_pack_host(self.c_params, bits_frame)

    def rans_unpack(self, coded, out=None) -> np.ndarray:
        """csic_rans_unpack_host: rANS-coded bytes -> a PLANAR_BITS frame buffer."""
        return rans_unpack_host(self.c_params, coded, out)

    # -- temporal delta coding of sequences of PLANAR_BITS frames (csic_delta_*) -------------------------
    @property
    def delta_layout(self) -> N.CsicDeltaLayout:
        """csic_delta_layout of these parameters: groups, the map's section offsets, map_bytes, map_stride."""
        return delta_layout(self.c_params)

    @property
    def delta_kernel_name(self) -> str:
        return N.lib().csic_delta_kernel_name(self._h).decode()

    def _temporal_buffers(self, ms, d_a, nframes, d_b, d_maps, what):
        """Both temporal layers: the frames of one side checked, the other side's and the maps (`ms`: the layer's map_stride) allocated
        unless given (csic_delta_*: `d_b` may be `d_a`, in place; csic_mc_*: the library refuses that)."""
        import torch
        fb = self.planar_bits_layout.frame_bytes
        self._pack_check(d_a, nframes * fb, what)
        if d_b is None:
            d_b = torch.empty((nframes, fb), dtype=torch.uint8, device=d_a.device)
        else:
            self._pack_check(d_b, nframes * fb, "the output frames")
        if d_maps is None:
            d_maps = torch.zeros((nframes, ms), dtype=torch.uint8, device=d_a.device)
        else:
            self._pack_check(d_maps, nframes * ms, "d_maps")
        return d_b, d_maps

    def delta_device(self, d_frames, nframes: int = 1, gop: int = 1, d_diff=None, d_maps=None):
        """d_frames: nframes PLANAR_BITS frame buffers on the device (frame_bytes each).  Returns (diff, maps): the difference frames, a
        uint8 tensor (nframes, frame_bytes) of which only the payload ranges are written -- `d_diff` may be `d_frames` itself, in place --
        and the maps, uint8 (nframes, map_stride) with map_bytes of each row written.  Either coder then packs `diff` as it packs
        frames.  Asynchronous on torch's current stream."""
        d_diff, d_maps = self._temporal_buffers(self.delta_layout.map_stride, d_frames, nframes, d_diff, d_maps, "d_frames")
        N.check(N.lib().csic_delta_device(self._h, C.c_void_p(d_frames.data_ptr()), int(nframes), int(gop), C.c_void_p(d_diff.data_ptr()),
                                          C.c_void_p(d_maps.data_ptr()), self._stream()))
        return d_diff, d_maps

    def undelta_device(self, d_diff, d_maps, nframes: int = 1, gop: int = 1, d_frames=None):
        """The inverse of delta_device (`d_frames` may be `d_diff`, in place).  The device does not validate the maps: check untrusted
        ones with undelta() first."""
        if d_maps is None:
            raise N.IllegalArgumentException(N.EINVAL_NULL, "requirement failed: d_maps is None")
        d_frames, _ = self._temporal_buffers(self.delta_layout.map_stride, d_diff, nframes, d_frames, d_maps, "d_diff")
        N.check(N.lib().csic_undelta_device(self._h, C.c_void_p(d_diff.data_ptr()), C.c_void_p(d_maps.data_ptr()), int(nframes), int(gop),
                                            C.c_void_p(d_frames.data_ptr()), self._stream()))
        return d_frames

    def delta(self, frames, gop: int, out=None):
        """csic_delta_host: frame buffers in host memory (nframes, frame_bytes) -> (diff, maps).  Needs no GPU."""
        return delta_host(self.c_params, frames, gop, out)

    def undelta(self, diff, maps, gop: int, out=None) -> np.ndarray:
        """csic_undelta_host: the inverse; damaged maps raise CsicIOError."""
        return undelta_host(self.c_params, diff, maps, gop, out)

    # -- motion-compensated delta coding of sequences of PLANAR_BITS frames (csic_mc_*) ------------------
    @property
    def mc_layout(self) -> N.CsicMcLayout:
        """csic_mc_layout of these parameters: groups, row widths, the map's table and section offsets, map_bytes, map_stride,
        workspace_frame_bytes."""
        return mc_layout(self.c_params)

    @property
    def mc_kernel_name(self) -> str:
        return N.lib().csic_mc_kernel_name(self._h).decode()

    def mc_delta_device(self, d_frames, nframes: int = 1, gop: int = 1, motion: int = 2, d_diff=None, d_maps=None, d_workspace=None):
        """As delta_device with displacements of up to `motion` samples either way (0..7): returns (diff, maps), the difference frames
        -- not in place: `d_diff` must lie apart from `d_frames` -- and the maps, uint8 (nframes, mc_layout.map_stride).  `d_workspace`:
        nframes * mc_layout.workspace_frame_bytes bytes for the vote counters, allocated unless given.  Asynchronous on torch's current
        stream."""
        import torch
        d_diff, d_maps = self._temporal_buffers(self.mc_layout.map_stride, d_frames, nframes, d_diff, d_maps, "d_frames")
        wsb = nframes * self.mc_layout.workspace_frame_bytes
        if d_workspace is None:
            d_workspace = torch.empty((wsb,), dtype=torch.uint8, device=d_frames.device)
        else:
            self._pack_check(d_workspace, wsb, "d_workspace")
        N.check(N.lib().csic_mc_delta_device(self._h, C.c_void_p(d_frames.data_ptr()), int(nframes), int(gop), int(motion), C.c_void_p(d_diff.data_ptr()),
                                             C.c_void_p(d_maps.data_ptr()), C.c_void_p(d_workspace.data_ptr()), wsb, self._stream()))
        return d_diff, d_maps

    def mc_undelta_device(self, d_diff, d_maps, nframes: int = 1, gop: int = 1, d_frames=None):
        """The inverse of mc_delta_device, one launch per step of a run.  The device does not validate the maps: check untrusted ones
        with mc_undelta() first."""
        if d_maps is None:
            raise N.IllegalArgumentException(N.EINVAL_NULL, "requirement failed: d_maps is None")
        d_frames, _ = self._temporal_buffers(self.mc_layout.map_stride, d_diff, nframes, d_frames, d_maps, "d_diff")
        N.check(N.lib().csic_mc_undelta_device(self._h, C.c_void_p(d_diff.data_ptr()), C.c_void_p(d_maps.data_ptr()), int(nframes), int(gop),
                                               C.c_void_p(d_frames.data_ptr()), self._stream()))
        return d_frames

    def mc_delta(self, frames, gop: int, motion: int, out=None):
        """csic_mc_delta_host: frame buffers in host memory (nframes, frame_bytes) -> (diff, maps).  Needs no GPU."""
        return mc_delta_host(self.c_params, frames, gop, motion, out)

    def mc_undelta(self, diff, maps, gop: int, out=None) -> np.ndarray:
        """csic_mc_undelta_host: the inverse; damaged maps raise CsicIOError."""
        return mc_undelta_host(self.c_params, diff, maps, gop, out)

    # -- row prediction of PLANAR_BITS frames in front of a coder (csic_rows_*) ----------------------------
    @property
    def rows_layout(self) -> N.CsicRowsLayout:
        """csic_rows_layout of these parameters: groups, row widths, K, S, the map's section offsets, map_bytes, map_stride."""
        return rows_layout(self.c_params)

    @property
    def rows_kernel_name(self) -> str:
        return N.lib().csic_rows_kernel_name(self._h).decode()

    def rows_device(self, d_frames, nframes: int = 1, d_diff=None, d_maps=None):
        """d_frames: nframes PLANAR_BITS frame buffers on the device (frame_bytes each).  Returns (diff, maps): the difference frames, a
        uint8 tensor (nframes, frame_bytes) of which only the payload ranges are written -- not in place: `d_diff` must lie apart from
        `d_frames` -- and the maps, uint8 (nframes, rows_layout.map_stride) with map_bytes of each row written.  Any coder then packs
        `diff` as it packs frames.  Asynchronous on torch's current stream."""
        d_diff, d_maps = self._temporal_buffers(self.rows_layout.map_stride, d_frames, nframes, d_diff, d_maps, "d_frames")
        N.check(N.lib().csic_rows_device(self._h, C.c_void_p(d_frames.data_ptr()), int(nframes), C.c_void_p(d_diff.data_ptr()),
                                         C.c_void_p(d_maps.data_ptr()), self._stream()))
        return d_diff, d_maps

    def unrows_device(self, d_diff, d_maps, nframes: int = 1, d_frames=None):
        """The inverse of rows_device (`d_frames` may be `d_diff`, in place).  The device does not validate the maps: check untrusted
        ones with unrows() first."""
        if d_maps is None:
            raise N.IllegalArgumentException(N.EINVAL_NULL, "requirement failed: d_maps is None")
        d_frames, _ = self._temporal_buffers(self.rows_layout.map_stride, d_diff, nframes, d_frames, d_maps, "d_diff")
        N.check(N.lib().csic_unrows_device(self._h, C.c_void_p(d_diff.data_ptr()), C.c_void_p(d_maps.data_ptr()), int(nframes),
                                           C.c_void_p(d_frames.data_ptr()), self._stream()))
        return d_frames

    def rows(self, frames, out=None):
        """csic_rows_host: frame buffers in host memory (nframes, frame_bytes) -> (diff, maps).  Needs no GPU."""
        return rows_host(self.c_params, frames, out)

    def unrows(self, diff, maps, out=None) -> np.ndarray:
        """csic_unrows_host: the inverse; damaged maps raise CsicIOError."""
        return unrows_host(self.c_params, diff, maps, out)

    # -- compute ----------------------------------------------------------------------------------
    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def process_device(self, d_in, d_out=None, nframes: int = 1):
        """d_in: CUDA int32/uint32 tensor with nframes*W*H elements (any shape).  Returns d_out shaped
        (Ho, Wo) or (nframes, Ho, Wo).  Asynchronous on torch's current stream."""
        import torch
        if not d_in.is_cuda or d_in.element_size() != 4 or not d_in.is_contiguous():
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_in must be a contiguous 4-byte CUDA tensor")
        if d_in.device.index != self.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: tensor is on a different device than the plan")
        if d_in.numel() != nframes * self.width * self.height:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: expected {nframes * self.width * self.height} input pixels, got {d_in.numel()}")
        if self.planar or self.planar_bits:
            # planar frame buffers: frame_bytes bytes per frame (csic_planar_layout / csic_planar_bits_layout), a uint8 tensor
            # (nframes, frame_bytes)
            fb = self.frame_bytes
            if d_out is None:
                d_out = torch.empty((nframes, fb) if nframes > 1 else (fb,), dtype=torch.uint8, device=d_in.device)
            elif d_out.numel() * d_out.element_size() != nframes * fb or not d_out.is_contiguous() or d_out.device != d_in.device:
                raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_out must hold nframes * planar_layout.frame_bytes bytes")
        else:
            shape = (self.out_height, self.out_width) if nframes == 1 else (nframes, self.out_height, self.out_width)
            if d_out is None:
                d_out = torch.empty(shape, dtype=d_in.dtype, device=d_in.device)
            elif d_out.numel() != nframes * self.out_width * self.out_height or not d_out.is_contiguous() \
                    or d_out.element_size() != 4 or d_out.device != d_in.device:
                raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_out has the wrong size/layout")
        if nframes == 1:
            st = N.lib().csic_process_device(self._h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), self._stream())
        else:
            st = N.lib().csic_process_batch_device(self._h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                                   nframes, self._stream())
        N.check(st)
        return d_out

    def process_device_pitched(self, d_in, in_pitch_px: int, d_out, out_pitch_px: int, nframes: int = 1,
                               in_offset_px: int = 0, out_offset_px: int = 0):
        """Frames whose rows are not tightly packed (csic_process_pitched_device): row r starts `in_pitch_px`
        pixels after row r-1.  `d_in` / `d_out` are 4-byte CUDA tensors that contain the (possibly padded or
        larger) surfaces; `*_offset_px` select the first pixel, e.g. the top-left corner of a region of interest.
        Asynchronous on torch's current stream; the caller guarantees the tensors are large enough."""
        need_in = in_offset_px + ((nframes * self.height - 1) * in_pitch_px + self.width)
        need_out = out_offset_px + ((nframes * self.out_height - 1) * out_pitch_px + self.out_width)
        if d_in.numel() < need_in or d_out.numel() < need_out or d_in.element_size() != 4 or d_out.element_size() != 4:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: surface too small for the pitched frame")
        N.check(N.lib().csic_process_pitched_device(
            self._h, C.c_void_p(d_in.data_ptr() + 4 * in_offset_px), in_pitch_px,
            C.c_void_p(d_out.data_ptr() + 4 * out_offset_px), out_pitch_px, nframes, self._stream()))
        return d_out

    def reconstruct_device(self, d_planar, d_out=None, nframes: int = 1, out_format: int = N.FMT_ARGB8888):
        """Planar frame buffers of these parameters -> packed pixels (csic_reconstruct_device): ARGB through the inverse
        transform, or the packed YCbCr stream.  reconstruct(planar(x)) == the packed output of the same parameters."""
        import torch
        fb = self.planar_layout.frame_bytes
        if not d_planar.is_cuda or not d_planar.is_contiguous() or d_planar.numel() * d_planar.element_size() != nframes * fb:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_planar must hold nframes * planar_layout.frame_bytes bytes")
        shape = (self.out_height, self.out_width) if nframes == 1 else (nframes, self.out_height, self.out_width)
        if d_out is None:
            d_out = torch.empty(shape, dtype=torch.int32, device=d_planar.device)
        elif d_out.numel() != nframes * self.out_width * self.out_height or d_out.element_size() != 4 or not d_out.is_contiguous():
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_out has the wrong size/layout")
        N.check(N.lib().csic_reconstruct_device(self._h, C.c_void_p(d_planar.data_ptr()), C.c_void_p(d_out.data_ptr()), nframes,
                                                int(out_format), self._stream()))
        return d_out

    def reconstruct_bits_device(self, d_bits, d_out=None, nframes: int = 1, out_format: int = N.FMT_ARGB8888):
        """Bit-packed planar frame buffers of these parameters -> packed pixels (csic_reconstruct_bits_device), as
        reconstruct_device does for PLANAR frames.  reconstruct_bits(bits(x)) == the packed output of the same parameters."""
        import torch
        fb = self.planar_bits_layout.frame_bytes
        if not d_bits.is_cuda or not d_bits.is_contiguous() or d_bits.numel() * d_bits.element_size() != nframes * fb:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_bits must hold nframes * planar_bits_layout.frame_bytes bytes")
        shape = (self.out_height, self.out_width) if nframes == 1 else (nframes, self.out_height, self.out_width)
        if d_out is None:
            d_out = torch.empty(shape, dtype=torch.int32, device=d_bits.device)
        elif d_out.numel() != nframes * self.out_width * self.out_height or d_out.element_size() != 4 or not d_out.is_contiguous():
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_out has the wrong size/layout")
        N.check(N.lib().csic_reconstruct_bits_device(self._h, C.c_void_p(d_bits.data_ptr()), C.c_void_p(d_out.data_ptr()), nframes,
                                                     int(out_format), self._stream()))
        return d_out

    # -- full-resolution decode (csic_decode_*) ---------------------------------------------------
    def _decode_src_bytes(self, src_format: int) -> int:
        """Bytes of one source frame of csic_decode_* in `src_format`."""
        if src_format == N.FMT_PLANAR_BITS:
            return self.planar_bits_layout.frame_bytes
        if src_format == N.FMT_PLANAR:
            return self.planar_layout.frame_bytes
        return 4 * self.out_width * self.out_height

    def decode_kernel_name(self, src_format: int, out_format: int = N.FMT_ARGB8888) -> str:
        """The kernel decode_device takes for 16-byte aligned buffers (csic_decode_kernel_name); "" for a refused pair."""
        return N.lib().csic_decode_kernel_name(self._h, int(src_format), int(out_format)).decode()

    def decode_device(self, d_src, src_format=None, d_out=None, nframes: int = 1, out_format: int = N.FMT_ARGB8888):
        """A compressed frame -> width x height packed pixels, decode(r, c) = o(r / f, c / f) (csic_decode_device).  d_src: a
        contiguous CUDA tensor holding nframes sources in `src_format` -- PLANAR_BITS / PLANAR frame buffers, or out_width *
        out_height packed YCBCR888X / ARGB8888 pixels per frame; None = the plan's own out_format.  Returns d_out shaped (H, W)
        or (nframes, H, W), int32.  Asynchronous on torch's current stream."""
        import torch
        src_format = self.c_params.out_format if src_format is None else int(src_format)
        if src_format not in (N.FMT_ARGB8888, N.FMT_YCBCR888X, N.FMT_PLANAR, N.FMT_PLANAR_BITS):
            raise N.IllegalArgumentException(N.EINVAL_FORMAT, f"requirement failed: unknown source format {src_format}")
        if not d_src.is_cuda or not d_src.is_contiguous() or d_src.numel() * d_src.element_size() != nframes * self._decode_src_bytes(src_format):
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_src must be a contiguous CUDA tensor of nframes source frames")
        if d_src.device.index != self.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: tensor is on a different device than the plan")
        shape = (self.height, self.width) if nframes == 1 else (nframes, self.height, self.width)
        if d_out is None:
            d_out = torch.empty(shape, dtype=torch.int32, device=d_src.device)
        elif d_out.numel() != nframes * self.width * self.height or d_out.element_size() != 4 or not d_out.is_contiguous() \
                or d_out.device != d_src.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_out has the wrong size/layout")
        N.check(N.lib().csic_decode_device(self._h, C.c_void_p(d_src.data_ptr()), src_format, C.c_void_p(d_out.data_ptr()),
                                           int(out_format), int(nframes), self._stream()))
        return d_out

    def decode_host(self, src: np.ndarray, src_format=None, nframes: int = 1, out_format: int = N.FMT_ARGB8888) -> np.ndarray:
        """csic_decode_host: nframes source frames in host memory -> uint32 array (H, W) or (nframes, H, W)."""
        src_format = self.c_params.out_format if src_format is None else int(src_format)
        a = np.ascontiguousarray(src).reshape(-1).view(np.uint8)
        out = np.empty(nframes * self.width * self.height, dtype=np.uint32)
        N.check(N.lib().csic_decode_host(self._h, a.ctypes.data_as(C.c_void_p), a.size, src_format, out.ctypes.data_as(C.c_void_p),
                                         out.size, int(out_format), int(nframes)))
        return out.reshape((self.height, self.width) if nframes == 1 else (nframes, self.height, self.width))

    def decode(self, src, src_format=None, nframes: int = 1, out_format: int = N.FMT_ARGB8888):
        if _is_torch_tensor(src):
            return self.decode_device(src, src_format, None, nframes, out_format)
        return self.decode_host(src, src_format, nframes, out_format)

    # -- view decode (csic_decode_view_*) ---------------------------------------------------------
    @staticmethod
    def _c_view(view) -> "N.CsicView":
        return N.CsicView(*(int(x) for x in View(*view)))

    def decode_view_kernel_name(self, src_format: int, view, out_format: int = N.FMT_ARGB8888) -> str:
        """The kernel decode_view_device takes for 16-byte aligned buffers (csic_decode_view_kernel_name); "" for a refused pair or view."""
        return N.lib().csic_decode_view_kernel_name(self._h, int(src_format), int(out_format), C.byref(self._c_view(view))).decode()

    def decode_view_device(self, d_src, view, src_format=None, d_out=None, nframes: int = 1, out_format: int = N.FMT_ARGB8888):
        """A compressed frame -> the window `view` of its decode, reduced by a scale x scale box (csic_decode_view_device): view.width
        x view.height packed pixels, each the rounded mean of the decoded pixels under its box; scale 1 is a crop.  d_src and
        src_format as for decode_device.  Returns d_out shaped (view.height, view.width) or (nframes, ...), int32.  Asynchronous on
        torch's current stream."""
        import torch
        view = View(*view)
        src_format = self.c_params.out_format if src_format is None else int(src_format)
        if src_format not in (N.FMT_ARGB8888, N.FMT_YCBCR888X, N.FMT_PLANAR, N.FMT_PLANAR_BITS):
            raise N.IllegalArgumentException(N.EINVAL_FORMAT, f"requirement failed: unknown source format {src_format}")
        if not d_src.is_cuda or not d_src.is_contiguous() or d_src.numel() * d_src.element_size() != nframes * self._decode_src_bytes(src_format):
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_src must be a contiguous CUDA tensor of nframes source frames")
        if d_src.device.index != self.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: tensor is on a different device than the plan")
        if view.width < 1 or view.height < 1:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: a view has at least one pixel, got {view.width} x {view.height}")
        shape = (view.height, view.width) if nframes == 1 else (nframes, view.height, view.width)
        if d_out is None:
            d_out = torch.empty(shape, dtype=torch.int32, device=d_src.device)
        elif d_out.numel() != nframes * view.width * view.height or d_out.element_size() != 4 or not d_out.is_contiguous() \
                or d_out.device != d_src.device:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: d_out has the wrong size/layout")
        N.check(N.lib().csic_decode_view_device(self._h, C.c_void_p(d_src.data_ptr()), src_format, C.byref(self._c_view(view)),
                                                C.c_void_p(d_out.data_ptr()), int(out_format), int(nframes), self._stream()))
        return d_out

    def decode_view_host(self, src: np.ndarray, view, src_format=None, nframes: int = 1, out_format: int = N.FMT_ARGB8888) -> np.ndarray:
        """csic_decode_view_host: nframes source frames in host memory -> uint32 array (view.height, view.width) or (nframes, ...)."""
        view = View(*view)
        src_format = self.c_params.out_format if src_format is None else int(src_format)
        a = np.ascontiguousarray(src).reshape(-1).view(np.uint8)
        out = np.empty(nframes * max(view.width, 0) * max(view.height, 0), dtype=np.uint32)
        N.check(N.lib().csic_decode_view_host(self._h, a.ctypes.data_as(C.c_void_p), a.size, src_format, C.byref(self._c_view(view)),
                                              out.ctypes.data_as(C.c_void_p), out.size, int(out_format), int(nframes)))
        return out.reshape((view.height, view.width) if nframes == 1 else (nframes, view.height, view.width))

    def decode_view(self, src, view, src_format=None, nframes: int = 1, out_format: int = N.FMT_ARGB8888):
        if _is_torch_tensor(src):
            return self.decode_view_device(src, view, src_format, None, nframes, out_format)
        return self.decode_view_host(src, view, src_format, nframes, out_format)

    def unpack_planar_bits(self, buf) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """One bit-packed planar frame buffer (bytes on the host) -> (Y (Ho, Wo), Cb, Cr) with the restored 8-bit values
        (code << (8 - q)): what split_planar gives for the PLANAR frame of the same parameters."""
        lay = self.planar_bits_layout
        b = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
        g = lay.geometry

        def plane(off, nbytes, count, q):
            bits = np.unpackbits(b[off:off + nbytes], bitorder="little")[:count * q].reshape(count, q)
            codes = (bits.astype(np.uint16) << np.arange(q, dtype=np.uint16)).sum(axis=1)
            return (codes << (8 - q)).astype(np.uint8)

        n = g.y_width * g.y_height
        return (plane(lay.y_offset, lay.y_bytes, n, lay.y_bits).reshape(g.y_height, g.y_width),
                plane(lay.cb_offset, lay.cb_bytes, g.chroma_samples, lay.cb_bits),
                plane(lay.cr_offset, lay.cr_bytes, g.chroma_samples, lay.cr_bits))

    def split_planar(self, buf) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """One planar frame buffer (bytes on the host: numpy uint8, or anything np.frombuffer takes) -> (Y (Ho, Wo), Cb, Cr):
        the chroma planes as flat arrays of planar_layout.chroma_samples values in sample order."""
        lay = self.planar_layout
        b = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
        n = lay.y_width * lay.y_height
        return (b[lay.y_offset:lay.y_offset + n].reshape(lay.y_height, lay.y_width),
                b[lay.cb_offset:lay.cb_offset + lay.chroma_samples], b[lay.cr_offset:lay.cr_offset + lay.chroma_samples])

    def process_host(self, argb: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(argb, dtype=np.uint32).reshape(-1)
        if self.planar or self.planar_bits:
            out = np.zeros(self.frame_bytes // 4, dtype=np.uint32)
            N.check(N.lib().csic_process_host(self._h, a.ctypes.data_as(C.c_void_p), a.size, out.ctypes.data_as(C.c_void_p), out.size))
            return out.view(np.uint8)
        out = np.empty(self.out_width * self.out_height, dtype=np.uint32)
        N.check(N.lib().csic_process_host(self._h, a.ctypes.data_as(C.c_void_p), a.size,
                                          out.ctypes.data_as(C.c_void_p), out.size))
        return out.reshape(self.out_height, self.out_width)

    def process(self, frame):
        return self.process_device(frame) if _is_torch_tensor(frame) else self.process_host(frame)


class FrameGraph:
    """Pre-recorded per-frame launches of one plan (csic_frame_graph_*; BASELINE.json configs[4]).

    `d_ins[k]` / `d_outs[k]` are CUDA tensors holding frame k's W*H input pixels / receiving its Wo*Ho output
    pixels; they may live anywhere on the plan's device (views into one big tensor, or separate allocations).
    backend "auto" (default; csic_frame_graph_create): the library's choice -- today always "fused"; `backend` then names
    what was picked.
    backend "hip": `branches` hipGraph chains, launch(stream) is asynchronous and ordered with the stream.
    backend "direct": AQL packets without barrier bits on the library's own user-mode queues (`branches` =
    queues); submit() starts immediately and returns a ticket, wait() blocks the host; launch(stream) is
    asynchronous and ordered with the stream on the device when `stream_ordered` (HIP signal memory shared with
    the queues), else the synchronous composition stream-sync + submit + wait.  launch() never uses more than 3 queues
    (`launch_branches`), whatever `branches` says: a fourth beside the launch stream's own queue gets time-sliced; it
    cannot be captured into a hipGraph (CsicRuntimeError, CSIC_ECAPTURE).
    backend "fused": not per-frame launches -- one kernel launch over all frames through a device-resident pointer
    table (frames in separate buffers at the speed of the contiguous batched launch); launch(stream) is an ordinary
    asynchronous launch."""

    BACKENDS = {"hip": N.FRAME_GRAPH_HIP, "direct": N.FRAME_GRAPH_DIRECT, "fused": N.FRAME_GRAPH_FUSED, "auto": N.FRAME_GRAPH_AUTO}

    def __init__(self, plan: Plan, d_ins, d_outs, branches=None, backend: str = "auto"):
        n = len(d_ins)
        if n != len(d_outs) or n == 0:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: need as many output as input frames (> 0)")
        if backend not in self.BACKENDS:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: backend must be one of {sorted(self.BACKENDS)}")
        # a planar plan's outputs are planar frame buffers (frame_bytes each, any 1- or 4-byte dtype; fused backend only)
        out_bytes = plan.planar_layout.frame_bytes if plan.planar else 4 * plan.out_width * plan.out_height
        for t_in, t_out in zip(d_ins, d_outs):
            if t_in.numel() != plan.width * plan.height or t_out.numel() * t_out.element_size() != out_bytes \
                    or t_in.element_size() != 4 or (t_out.element_size() != 4 and not plan.planar) \
                    or not t_in.is_contiguous() or not t_out.is_contiguous() \
                    or t_in.device.index != plan.device or t_out.device.index != plan.device:
                raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: frame tensor has the wrong size/layout/device")
        self.plan, self.device, self.backend = plan, plan.device, backend
        self._keep = (list(d_ins), list(d_outs))              # the graph holds raw pointers
        pin = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in d_ins])
        pout = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in d_outs])
        self._h = C.c_void_p()
        N.check(N.lib().csic_frame_graph_create_ex(plan._h, pin, pout, n, 0 if branches is None else int(branches),
                                                   self.BACKENDS[backend], C.byref(self._h)))
        nf, nb = C.c_int32(), C.c_int32()
        N.check(N.lib().csic_frame_graph_count(self._h, C.byref(nf), C.byref(nb)))
        self.nframes, self.branches = nf.value, nb.value
        resolved = N.lib().csic_frame_graph_backend(self._h)
        self.requested_backend = backend
        self.backend = next(k for k, v in self.BACKENDS.items() if v == resolved)
        self.launch_branches = N.lib().csic_frame_graph_launch_branches(self._h)
        self.stream_ordered = bool(N.lib().csic_frame_graph_stream_ordered(self._h))

    def launch(self, stream=None) -> None:
        """Replays the graph on `stream` (a torch.cuda.Stream; default: torch's current stream), ordered with it.
        Asynchronous when `stream_ordered`."""
        import torch
        s = torch.cuda.current_stream(self.device) if stream is None else stream
        N.check(N.lib().csic_frame_graph_launch(self._h, C.c_void_p(s.cuda_stream)))

    def submit(self) -> int:
        """backend "direct": start all frames now (inputs must be ready); returns a ticket for wait()."""
        t = C.c_int64()
        N.check(N.lib().csic_frame_graph_submit(self._h, C.byref(t)))
        return t.value

    def wait(self, ticket: int = -1) -> None:
        """backend "direct": block until submission `ticket` (default: every submission so far) has finished."""
        N.check(N.lib().csic_frame_graph_wait(self._h, ticket))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            N.lib().csic_frame_graph_destroy(self._h)
            self._h = C.c_void_p()
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ImageCompressorTop:
    """RGB2YCbCr -> op1 -> op2 -> op3 (-> YCbCr2RGB), parameter list of ImageCompressorTop.scala:11-25."""

    def __init__(self, width: int, height: int,
                 chroma_param_a_config: int, chroma_param_b_config: int,
                 yTargetQuantBitsConfig: int, cbTargetQuantBitsConfig: int, crTargetQuantBitsConfig: int,
                 downFactorConfig: int,
                 op1Type: ProcessingStep, op2Type: ProcessingStep, op3Type: ProcessingStep,
                 *, rounding: Rounding = Rounding.FLOOR_HW, device: int = 0,
                 sampling: Sampling = Sampling.HOLD_DECIMATE):
        self.width, self.height = width, height
        self.ops = (ProcessingStep(op1Type), ProcessingStep(op2Type), ProcessingStep(op3Type))
        self.rounding, self.device = Rounding(rounding), device
        self.sampling = Sampling(sampling)       # AVG = extension without a reference counterpart
        self._args = (width, height, chroma_param_a_config, chroma_param_b_config, yTargetQuantBitsConfig,
                      cbTargetQuantBitsConfig, crTargetQuantBitsConfig, downFactorConfig, self.ops)
        # construction-time require()s, before any device is touched (ImageCompressorTop.scala:27-31 etc.)
        N.check(N.lib().csic_validate(C.byref(self._c_params(PixelFormat.ARGB8888))))
        self._plans = {}

    def _c_params(self, fmt: PixelFormat) -> N.CsicParams:
        return make_c_params(*self._args, rounding=self.rounding, out_format=fmt, strict_divisible=False,
                             sampling=self.sampling)

    def plan(self, fmt: PixelFormat = PixelFormat.ARGB8888) -> Plan:
        if fmt not in self._plans:
            self._plans[fmt] = Plan(self._c_params(fmt), self.device)
        return self._plans[fmt]

    @property
    def out_dims(self) -> Tuple[int, int]:
        """(out_width, out_height) = ceil(W/f), ceil(H/f): what SpatialDownsampler emits."""
        wo, ho = C.c_int32(), C.c_int32()
        N.check(N.lib().csic_out_dims(C.byref(self._c_params(PixelFormat.ARGB8888)), C.byref(wo), C.byref(ho)))
        return wo.value, ho.value

    def process(self, argb):
        """ARGB frame in -> reconstructed ARGB frame out (what ImageCompressionApp writes to the PNG:
        the DUT's YCbCr output put through YCbCrUtils.ycbcr2rgb, ImageCompressorTopApp.scala:118)."""
        return self.plan(PixelFormat.ARGB8888).process(argb)

    def processYCbCr(self, argb):
        """ARGB frame in -> the PixelYCbCrBundle stream io.out carries (byte0=Y, byte1=Cb, byte2=Cr)."""
        return self.plan(PixelFormat.YCBCR888X).process(argb)

    def distortion(self, argb):
        """What these parameters cost in image quality on `argb` (one frame, or a stack (n, H, W)): Distortion (list of them for a
        stack) -- the per-channel sums of squared errors against the packed ARGB / YCbCr outputs and their PSNR."""
        return self.plan(PixelFormat.ARGB8888).distortion(argb)

    def ssim(self, argb):
        """How much of the structure of `argb` (one frame, or a stack (n, H, W)) these parameters keep: Ssim (list of them for a
        stack) -- the per-channel 8 x 8 block SSIM against the packed ARGB / YCbCr outputs."""
        return self.plan(PixelFormat.ARGB8888).ssim(argb)

    def qsweep(self, argb) -> QSweep:
        """Rate and distortion of every (y, cb, cr) bit set of these parameters on `argb` (one frame, or a stack (n, H, W)) from one
        pass: QSweep (csic_qsweep_*).  The three bit widths this compressor was built with do not matter."""
        return self.plan(PixelFormat.ARGB8888).qsweep(argb)

    def codeStats(self, argb):
        """What the samples of `argb`'s compressed frame really carry: CodeStats of its bit-packed planes (csic_code_stats_*).  A
        CUDA frame is compressed and measured on the device with no host round trip in between; a numpy frame goes through the
        two host entry points."""
        pl = self.plan(PixelFormat.PLANAR_BITS)
        return pl.code_stats(pl.process(argb))

    def processPlanarBits(self, argb):
        """ARGB frame in -> one bit-packed planar frame buffer (CSIC_FMT_PLANAR_BITS, uint8: planar_bits_layout.frame_bytes on the
        host, a CUDA uint8 tensor for a CUDA input); Plan.unpack_planar_bits cuts it into the three planes."""
        return self.plan(PixelFormat.PLANAR_BITS).process(argb)

    def decode(self, buf):
        """One bit-packed planar frame buffer (what processPlanarBits returns: host bytes or a CUDA uint8 tensor) -> the ARGB frame
        of the ORIGINAL size, height x width: every reconstructed pixel replicated factor x factor times (csic_decode_*)."""
        return self.plan(PixelFormat.PLANAR_BITS).decode(buf)

    def decodeView(self, buf, view):
        """One bit-packed planar frame buffer -> the ARGB pixels of `view` (a View: x0, y0, width, height in output pixels, scale):
        the window of decode(buf) that starts at (x0, y0), reduced by a scale x scale box (csic_decode_view_*).  The whole frame is
        never written."""
        return self.plan(PixelFormat.PLANAR_BITS).decode_view(buf, view)

    def close(self) -> None:
        for p in self._plans.values():
            p.close()
        self._plans = {}


class ImageProcessor(ImageCompressorTop):
    """Fixed pipeline RGB2YCbCr -> ChromaSubsampler -> SpatialDownsampler, no quantiser
    (ImageProcessor.scala:42-62)."""

    def __init__(self, p: ImageProcessorParams, *, rounding: Rounding = Rounding.FLOOR_HW, device: int = 0):
        if not isinstance(p, ImageProcessorParams):
            raise TypeError("ImageProcessor takes an ImageProcessorParams")
        self.p = p
        super().__init__(p.width, p.height, p.chromaParamA, p.chromaParamB, 8, 8, 8, p.factor,
                         ProcessingStep.ChromaSubsampling, ProcessingStep.SpatialSampling,
                         ProcessingStep.ColorQuantization, rounding=rounding, device=device)
