"""MI355X-native drop-in for the pixel-stream hot path of Andurdur/Chroma-Subsampling-Image-Compressor.

The compute lives in libcsic_hip.so (csrc/, hand-written HIP for gfx950) behind the C ABI of
include/csic.h; this package is the host-side mirror of the reference's generator surface
(ImageProcessorParams / ProcessingStep / ImageCompressorTop / ImageProcessor / ImageProcessorModel /
ImageCompressionApp).  There is no CPU compute path in here.
"""
from . import _native
from ._native import CsicIOError, CsicRuntimeError, IllegalArgumentException
from .params import ImageProcessorParams, PixelFormat, ProcessingStep, Rounding, Sampling, make_c_params
from .compressor import CodeStats, Distortion, FrameGraph, ImageCompressorTop, ImageProcessor, Plan, QSweep, Ssim, View
from .model import Image, ImageProcessorModel
from .pipeline import FramePipeline
from .stages import (ChromaSubsampler, ColorQuantizer, PixelBundle, PixelYCbCrBundle, ReferenceModel, RGB2YCbCr,
                     SpatialDownsampler, YCbCrUtils, pack_ycc, unpack_ycc)
from .container import (container_coded_sizes, container_info, container_inter_groups, delta_host, delta_layout, undelta_host,
                        mc_delta_host, mc_layout, mc_undelta_host, rows_host, rows_layout, unrows_host, pack_frame_host, pack_layout, read_container, rans_layout, rans_pack_host,
                        rans_unpack_host, rice_layout, rice_pack_host, rice_unpack_host, unpack_frame_host, write_container, write_container_coded)
from .app import ImageCompressionApp
from .distributed import MultiDeviceCompressor, Stripe, StripedImageCompressorTop, halo_stripe_for_rank, stripe_for_rank
from . import app, compressor, container, distributed, model, params, pipeline, stages, stream

__all__ = [
    "CsicIOError", "CsicRuntimeError", "IllegalArgumentException", "ImageProcessorParams", "PixelFormat", "ProcessingStep",
    "Rounding", "Sampling", "make_c_params", "ImageCompressorTop", "ImageProcessor", "Plan", "FrameGraph", "Distortion", "Ssim", "CodeStats", "QSweep", "View", "Image", "ImageProcessorModel",
    "ImageCompressionApp", "FramePipeline", "ChromaSubsampler", "ColorQuantizer", "PixelBundle", "PixelYCbCrBundle", "ReferenceModel", "RGB2YCbCr",
    "SpatialDownsampler", "YCbCrUtils", "pack_ycc", "unpack_ycc", "Stripe", "StripedImageCompressorTop", "MultiDeviceCompressor", "halo_stripe_for_rank", "stripe_for_rank",
    "container_info", "read_container", "write_container", "write_container_coded", "container_coded_sizes", "pack_layout", "pack_frame_host",
    "unpack_frame_host", "rice_layout", "rice_pack_host", "rice_unpack_host", "rans_layout", "rans_pack_host", "rans_unpack_host", "delta_layout", "delta_host", "undelta_host",
    "mc_layout", "mc_delta_host", "mc_undelta_host", "rows_layout", "rows_host", "unrows_host", "container_inter_groups",
]
