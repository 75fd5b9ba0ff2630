"""Drop-in for `sbt "Test / runMain jpeg.ImageCompressionApp ..."`:

    python -m csic_amd.app --input test_images/in128x128.png --a 2 --b 0 --sf 2 --op1 chroma --op2 spatial --op3 color

ImageCompressionApp <- object ImageCompressionApp, src/test/scala/jpeg/ImageCompressorTopApp.scala:18-216
Same flags (space-separated `--key value` pairs, :149-151), same defaults (:164-173; note sf = 8 and the
order spatial, color, chroma), same banner, same output naming including the literal `order-Pr-Pr-Pr`
tag (:188; ChiselEnum.toString quirk).  The simulated-RTL run is replaced by one fused
HIP launch.

Two leading verbs go past what the reference's app does (it only ever writes the reconstructed pixels as a PNG):

    python -m csic_amd.app compress   --input x.png --output x.csic --a 2 --b 0 --yq 6 --cbq 5 --crq 5 --sf 2 ... [--coding raw|groups|rice|rans]
    python -m csic_amd.app compress   --input x.png --output x.csic --coding groups|rice|rans --rows ...      (row prediction in front of the coder: version 8)
    python -m csic_amd.app compress   --input x.png --output x.csic --target-bytes N [--coding raw|groups|rice|rans] [--yq 8 --cbq 8 --crq 8: upper bounds]
    python -m csic_amd.app compress   --inputs a.png,b.png,... --gop K [--motion R] --coding groups|rice|rans --output x.csic ...
    python -m csic_amd.app decompress --input x.csic --output x.png [--frame K | --output-pattern frame_%03d.png]
    python -m csic_amd.app decompress --input x.csic --output x.png [--window x,y,w,h] [--scale 1|2|4|8|16]    (a window of the frame, box-reduced: decompress --help)

    python -m csic_amd.app inspect    --input x.csic

`compress` writes the bit-packed planes as a .csic container (include/csic.h) -- as they are (`--coding raw`, the default: version 1)
or coded on the GPU (`--coding groups`: csic_pack_device, version 3; `--coding rice`: csic_rice_pack_device, version 4; both lossless, the
second smaller) --, or, with `--inputs` and `--gop`, frames of equal size as a sequence (csic_delta_device in front of the device
coder: version 5) --, `decompress` decodes any of them back
to a PNG of the original size (frame 0, `--frame K`, or every frame through `--output-pattern`), `inspect` prints a container's header, its coding and stored bytes per frame and, per frame, what its samples carry: the entropies of the codes and of
their left-predicted residuals and the sizes an entropy coder could reach (csic_code_stats_*).  The verb must be the first
argument; with any other first argument main() behaves as described above.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional

import numpy as np

from .compressor import ImageCompressorTop, Plan, View
from . import _native as N
from .container import (container_coded_sizes, container_info, container_inter_groups, delta_layout, mc_layout, rans_layout, read_container, rows_layout,
                        write_container, write_container_coded)
from .model import Image, ImageProcessorModel
from .params import PixelFormat, ProcessingStep, Sampling


class ImageCompressionApp:
    @staticmethod
    def processImage(inputImagePath: str, outputImagePath: str,
                     chromaParamA: int, chromaParamB: int,
                     yTargetBits: int, cbTargetBits: int, crTargetBits: int,
                     spatialFactorToUse: int,
                     op1: ProcessingStep, op2: ProcessingStep, op3: ProcessingStep, *, device: int = 0,
                     emulateCollectorBudget: bool = False) -> None:
        """ImageCompressorTopApp.scala:23-145.

        emulateCollectorBudget: the reference's collector loop gives up after (W/f)*(H/f)*40 + 10000 simulated cycles (:110)
        and the pixels it did not get keep the image's magenta fill (:133-141).  ImageCompressorTop accepts one pixel every
        two cycles (three non-pipe Queue(1)s), so that budget is too small for sf = 8 on anything larger than ~85x85 --
        including the app's own defaults (in128x128.png, sf = 8: 160 of 256 pixels).  Off (default), every pixel is
        written; on, the cycle-level model (stream.ImageCompressorTop) is asked how many pixels the collector would have
        got and the rest stays magenta, which is what a run of the reference app is predicted to produce.  The pixel
        VALUES come from the GPU either way; the model contributes a count."""
        inputImage = ImageProcessorModel.readImage(inputImagePath)
        W, H = inputImage.width, inputImage.height
        f = spatialFactorToUse
        spatial_in = ProcessingStep.SpatialSampling in (op1, op2, op3)
        top = ImageCompressorTop(W, H, chromaParamA, chromaParamB, yTargetBits, cbTargetBits, crTargetBits,
                                 f, op1, op2, op3, device=device)
        finalW = W // f if spatial_in else W                      # :44-45
        finalH = H // f if spatial_in else H
        if spatial_in and (W % f != 0 or H % f != 0):
            print(f"[WARN] Image dimensions ({W}x{H}) are not perfectly divisible by spatialFactor ({f}). "
                  "SpatialDownsampler might truncate.")                # :47-49
        out = top.process(inputImage.argb)                           # (ceil(H/f), ceil(W/f)) stream, row-major
        top.close()
        # The harness collects the first finalW*finalH pixels of the OUTPUT STREAM and lays them out
        # finalW per row (:108-124, :133-142); identical to `out` when the dimensions divide.
        stream = out.reshape(-1)[: finalW * finalH]
        if emulateCollectorBudget:
            from .stream import ImageCompressorTop as CycleModel
            with CycleModel(W, H, chromaParamA, chromaParamB, yTargetBits, cbTargetBits, crTargetBits, f, op1, op2, op3) as dut:
                got, _ = dut.run(inputImage.argb, max_out=finalW * finalH, max_cycles=dut.collection_budget())
            if got.size < finalW * finalH:
                print(f"[WARN] Output collection timed out. Collected {got.size} out of {finalW * finalH} pixels.")    # :126-128
            stream = stream[: got.size]
        if stream.size < finalW * finalH:
            pad = np.full(finalW * finalH - stream.size, 0xFFFF00FF, dtype=np.uint32)   # AwtColor.MAGENTA fill, :133
            stream = np.concatenate([stream, pad])
        ImageProcessorModel.writeImage(Image(stream.reshape(finalH, finalW)), outputImagePath)


    @staticmethod
    def compressImage(inputImagePath: str, outputPath: str,
                      chromaParamA: int, chromaParamB: int,
                      yTargetBits: int, cbTargetBits: int, crTargetBits: int,
                      spatialFactorToUse: int,
                      op1: ProcessingStep, op2: ProcessingStep, op3: ProcessingStep,
                      sampling: Sampling = Sampling.HOLD_DECIMATE, *, device: int = 0, coding: str = "raw", rows: bool = False) -> int:
        """PNG -> CSIC_FMT_PLANAR_BITS plan -> .csic container.  Returns the bytes written (coding "raw": 80 + payload_bytes;
        "groups" / "rice" / "rans": the frame is coded on the device and goes out through csic_container_write_coded_ex).  rows: the
        row-prediction layer (csic_rows_device) in front of the coder, version 8; it needs a coding other than "raw"."""
        if coding not in ("raw", "groups", "rice", "rans"):
            raise N.IllegalArgumentException(N.EINVAL_FORMAT, f"requirement failed: --coding must be rans, raw, groups or rice, got {coding!r}")
        if rows and coding == "raw":
            raise N.IllegalArgumentException(N.EINVAL_FORMAT, "requirement failed: --rows needs --coding rans, groups or rice: the layer gains nothing without a coder")
        inputImage = ImageProcessorModel.readImage(inputImagePath)
        return ImageCompressionApp._compressFrame(inputImage, outputPath, chromaParamA, chromaParamB, yTargetBits, cbTargetBits, crTargetBits,
                                                  spatialFactorToUse, op1, op2, op3, sampling, device, coding, rows)

    @staticmethod
    def _compressFrame(inputImage, outputPath, chromaParamA, chromaParamB, yTargetBits, cbTargetBits, crTargetBits, spatialFactorToUse,
                       op1, op2, op3, sampling, device, coding, rows=False) -> int:
        """compressImage behind its argument check and its PNG reader."""
        top = ImageCompressorTop(inputImage.width, inputImage.height, chromaParamA, chromaParamB, yTargetBits, cbTargetBits,
                                 crTargetBits, spatialFactorToUse, op1, op2, op3, device=device, sampling=sampling)
        try:
            plan = top.plan(PixelFormat.PLANAR_BITS)
            os.makedirs(os.path.dirname(os.path.abspath(outputPath)), exist_ok=True)
            if coding != "raw":
                import torch
                d_in = torch.from_numpy(np.ascontiguousarray(inputImage.argb, dtype=np.uint32).reshape(-1).view(np.int32)).to(f"cuda:{device}")
                pack = {"groups": plan.pack_device, "rice": plan.rice_pack_device, "rans": plan.rans_pack_device}[coding]
                bits = plan.process_device(d_in)
                maps = None
                if rows:                                    # the difference frame is what the coder packs
                    bits, maps = plan.rows_device(bits.reshape(1, plan.frame_bytes))
                coded, sizes = pack(bits)
                write_container_coded(outputPath, plan.c_params, coded.cpu().numpy(), sizes.cpu().numpy(), coding=coding,
                                      maps=None if maps is None else maps.cpu().numpy(), rows=rows)
            else:
                bits = plan.process_host(inputImage.argb)
                write_container(outputPath, plan.c_params, bits)
        finally:
            top.close()
        return os.path.getsize(outputPath)

    @staticmethod
    def compressImageToSize(inputImagePath: str, outputPath: str,
                            chromaParamA: int, chromaParamB: int,
                            yMaxBits: int, cbMaxBits: int, crMaxBits: int,
                            spatialFactorToUse: int,
                            op1: ProcessingStep, op2: ProcessingStep, op3: ProcessingStep,
                            sampling: Sampling = Sampling.HOLD_DECIMATE, *, targetBytes: int, coding: str = "rans",
                            weights=(1, 1, 1), device: int = 0) -> dict:
        """PNG -> a .csic container of at most targetBytes bytes, with the bit widths (each at most yMaxBits / cbMaxBits / crMaxBits)
        of least distortion that the budget allows.  The procedure:
          1. Sweep the quantiser axis once (csic_qsweep_*), rank the bit sets (csic_qsweep_rank: ascending weighted distortion
             w_y sse_Y + w_cb sse_Cb + w_cr sse_Cr, then est_bytes) and set r = 1.
          2. Walk the candidates in rank order and skip those with est_bytes * r > targetBytes.
          3. If none is left before any encode, refuse with IllegalArgumentException and write no file.
          4. Encode the candidate with the device coder and the container writer, as compressImage does.
          5. If the file is <= targetBytes, it is done.
          6. Otherwise set r = max(r, size / est_bytes) and continue the walk behind that candidate.
          7. Make at most CSIC_QSWEEP_MAX_TRIES = 4 encodes; after that, or when the walk ends, remove the file and raise
             CsicRuntimeError ("not reachable in 4 tries").
        With coding "raw" est_bytes is the file's size, so the first candidate that fits is written in one try.
        Returns {"bits": (y, cb, cr), "est_bytes", "bytes", "tries", "psnr": (Y, Cb, Cr) from the sweep's table}."""
        if coding not in ("raw", "groups", "rice", "rans"):
            raise N.IllegalArgumentException(N.EINVAL_FORMAT, f"requirement failed: --coding must be rans, raw, groups or rice, got {coding!r}")
        targetBytes = int(targetBytes)
        if targetBytes < 80:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: --target-bytes must be at least the 80 bytes of a header, got {targetBytes}")
        inputImage = ImageProcessorModel.readImage(inputImagePath)
        top = ImageCompressorTop(inputImage.width, inputImage.height, chromaParamA, chromaParamB, 8, 8, 8, spatialFactorToUse, op1, op2, op3,
                                 device=device, sampling=sampling)
        try:
            sweep = top.qsweep(inputImage.argb)
        finally:
            top.close()
        ranked = sweep.rank(coding, weights, (yMaxBits, cbMaxBits, crMaxBits))
        r, tries = 1.0, 0
        for _, est, bits in ranked:
            if est * r > targetBytes:
                continue
            if tries == N.QSWEEP_MAX_TRIES:
                break
            size = ImageCompressionApp._compressFrame(inputImage, outputPath, chromaParamA, chromaParamB, *bits, spatialFactorToUse, op1, op2, op3,
                                                      sampling, device, coding)
            tries += 1
            if size <= targetBytes:
                return {"bits": bits, "est_bytes": est, "bytes": size, "tries": tries,
                        "psnr": tuple(sweep.psnr(p, q) for p, q in enumerate(bits))}
            r = max(r, size / est)
        if tries == 0:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: no bit set is estimated to fit {targetBytes} bytes "
                                             f"(the smallest estimate is {min(e for _, e, _ in ranked)} bytes)")
        os.remove(outputPath)
        raise N.CsicRuntimeError(N.EINVAL_SIZE, f"{targetBytes} bytes not reachable in {N.QSWEEP_MAX_TRIES} tries ({tries} encodes made)")

    @staticmethod
    def compressSequence(inputImagePaths, outputPath: str,
                         chromaParamA: int, chromaParamB: int,
                         yTargetBits: int, cbTargetBits: int, crTargetBits: int,
                         spatialFactorToUse: int,
                         op1: ProcessingStep, op2: ProcessingStep, op3: ProcessingStep,
                         sampling: Sampling = Sampling.HOLD_DECIMATE, *, device: int = 0, coding: str = "rice", gop: int = 16,
                         motion: Optional[int] = None) -> int:
        """PNGs of equal size -> one CSIC_FMT_PLANAR_BITS plan -> csic_delta_device -> the device coder -> a version-5 .csic container
        (csic_container_write_coded_seq); with a `motion` range csic_mc_delta_device and version 6; coding "rans": version 7 either way.
        Returns the bytes written."""
        if coding not in ("groups", "rice", "rans"):
            raise N.IllegalArgumentException(N.EINVAL_FORMAT, f"requirement failed: a sequence takes --coding rans, groups or rice, got {coding!r}")
        paths = list(inputImagePaths)
        if not paths:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: no input image")
        images = [ImageProcessorModel.readImage(p) for p in paths]
        W, H = images[0].width, images[0].height
        for p, im in zip(paths, images):
            if (im.width, im.height) != (W, H):
                raise N.IllegalArgumentException(N.EINVAL_DIMS, f"requirement failed: {p} is {im.width}x{im.height}, the sequence is {W}x{H}")
        top = ImageCompressorTop(W, H, chromaParamA, chromaParamB, yTargetBits, cbTargetBits, crTargetBits, spatialFactorToUse, op1, op2, op3,
                                 device=device, sampling=sampling)
        try:
            import torch
            plan = top.plan(PixelFormat.PLANAR_BITS)
            os.makedirs(os.path.dirname(os.path.abspath(outputPath)), exist_ok=True)
            n = len(images)
            argb = np.stack([np.ascontiguousarray(im.argb, dtype=np.uint32).reshape(-1) for im in images])
            d_in = torch.from_numpy(argb.reshape(-1).view(np.int32)).to(f"cuda:{device}")
            bits = plan.process_device(d_in, None, n).reshape(n, plan.frame_bytes)
            diff, maps = plan.delta_device(bits, n, gop) if motion is None else plan.mc_delta_device(bits, n, gop, motion)
            pack = {"groups": plan.pack_device, "rice": plan.rice_pack_device, "rans": plan.rans_pack_device}[coding]
            coded, sizes = pack(diff, n)
            write_container_coded(outputPath, plan.c_params, coded.cpu().numpy(), sizes.cpu().numpy(), coding=coding, maps=maps.cpu().numpy(), gop=gop,
                                  motion=motion)
        finally:
            top.close()
        return os.path.getsize(outputPath)

    @staticmethod
    def viewOf(width: int, height: int, window=None, scale: int = 1) -> Optional[View]:
        """The View of `decompress --window x,y,w,h --scale s` on a width x height frame: the window is in source pixels (default:
        the whole frame), the output is (w // s) x (h // s) pixels and the remainder of the window is dropped.  None when neither is
        given -- the plain decode.  A scale outside 1, 2, 4, 8, 16, a window outside the frame or smaller than one box is refused."""
        if window is None and scale == 1:
            return None
        if scale not in (1, 2, 4, 8, 16):
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: --scale must be 1, 2, 4, 8 or 16, got {scale}")
        x, y, w, h = (0, 0, width, height) if window is None else window
        if x < 0 or y < 0 or w < 1 or h < 1 or x + w > width or y + h > height:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: --window {x},{y},{w},{h} does not lie inside the {width}x{height} frame")
        if w < scale or h < scale:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: --window {x},{y},{w},{h} is smaller than one {scale}x{scale} box")
        return View(x, y, w // scale, h // scale, scale)

    @staticmethod
    def decompressImage(inputPath: str, outputImagePath: str, *, device: int = 0, frame: int = 0, window=None, scale: int = 1) -> None:
        """.csic container -> plan from the stored parameters -> csic_decode_* -> PNG of width x height: frame `frame` of a container
        that holds several (the first by default).  With a window (x, y, w, h in source pixels) or a scale: csic_decode_view_*, a PNG
        of (w // scale) x (h // scale) pixels (viewOf)."""
        c_params, nframes, frames = read_container(inputPath)
        if not 0 <= frame < nframes:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: --frame must be in 0..{nframes - 1}, got {frame}")
        view = ImageCompressionApp.viewOf(c_params.width, c_params.height, window, scale)
        with Plan(c_params, device) as plan:
            argb = plan.decode_host(frames[frame]) if view is None else plan.decode_view_host(frames[frame], view)
        ImageProcessorModel.writeImage(Image(argb), outputImagePath)

    @staticmethod
    def decompressImages(inputPath: str, outputPattern: str, *, device: int = 0, window=None, scale: int = 1) -> List[str]:
        """Every frame of a container to outputPattern % k (a printf pattern such as "frame_%03d.png"), whole or as the view of
        `window` and `scale` (decompressImage).  Returns the paths written."""
        c_params, nframes, frames = read_container(inputPath)
        paths = [outputPattern % k for k in range(nframes)]
        view = ImageCompressionApp.viewOf(c_params.width, c_params.height, window, scale)
        with Plan(c_params, device) as plan:
            for k, path in enumerate(paths):
                ImageProcessorModel.writeImage(Image(plan.decode_host(frames[k]) if view is None else plan.decode_view_host(frames[k], view)), path)
        return paths

    @staticmethod
    def processImages(inputImagePaths, outputImagePaths, chromaParamA: int, chromaParamB: int,
                      yTargetBits: int, cbTargetBits: int, crTargetBits: int, spatialFactorToUse: int,
                      op1: ProcessingStep, op2: ProcessingStep, op3: ProcessingStep, *, device: int = 0,
                      depth: int = 3, decodeThreads: int = None, encodeThreads: int = None, compression: int = 6):
        """Many same-sized images through one plan.  Output files are what processImage would write for each input.

        Default: csic_process_png_files -- pools of decoder and encoder threads inside the library (no GIL) around
        pinned frame slots; a decoder inflates a PNG straight into a slot and launches the kernel on the slot's stream,
        an encoder waits for the slot and writes the output file.  decodeThreads / encodeThreads = None: the library's
        choice; returns the call's csic_files_stats as a dict.
        decodeThreads=0: the serial reference flow of round 2 -- this thread decodes into a FramePipeline slot, submits,
        collects and encodes, one image after the other (only H2D / kernel / D2H of neighbouring images overlap); kept
        as the baseline the pooled path is byte-compared against (tests/test_gpu_parity.py)."""
        import ctypes as C
        from . import _native as N
        inputImagePaths, outputImagePaths = list(inputImagePaths), list(outputImagePaths)
        n = len(inputImagePaths)
        if n == 0:
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: no input image")
        if n != len(outputImagePaths):
            raise N.IllegalArgumentException(N.EINVAL_SIZE, "requirement failed: need as many output as input paths")
        W, H = ImageProcessorModel.imageSize(inputImagePaths[0])
        f = spatialFactorToUse
        finalW, finalH = W // f, H // f
        if finalW == 0 or finalH == 0:
            # the reference's collector would build a 0-pixel image (ImageCompressorTopApp.scala:44-45); there is nothing to write,
            # and a final size of 0 means "the plan's output size" to the C ABI -- refuse instead of writing something else
            raise N.IllegalArgumentException(N.EINVAL_SIZE, f"requirement failed: a {W}x{H} image at factor {f} leaves no whole output pixel")
        top = ImageCompressorTop(W, H, chromaParamA, chromaParamB, yTargetBits, cbTargetBits, crTargetBits,
                                 f, op1, op2, op3, device=device)
        try:
            for path in outputImagePaths:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)     # outputFile.getParentFile().mkdirs(), ImageProcessorModel.scala:20
            if decodeThreads == 0:
                ImageCompressionApp._processImagesSerial(top, inputImagePaths, outputImagePaths, finalW, finalH, depth, compression)
                return None
            ins = (C.c_char_p * n)(*[os.fsencode(p) for p in inputImagePaths])
            outs = (C.c_char_p * n)(*[os.fsencode(p) for p in outputImagePaths])
            st = N.CsicFilesStats()
            N.check(N.lib().csic_process_png_files(top.plan()._h, ins, outs, n, decodeThreads or 0, encodeThreads or 0, compression,
                                                   finalW, finalH, C.byref(st)))
            return {k: getattr(st, k) for k, _ in N.CsicFilesStats._fields_}
        finally:
            top.close()

    @staticmethod
    def _processImagesSerial(top, inputImagePaths, outputImagePaths, finalW, finalH, depth, compression):
        from .pipeline import FramePipeline
        todo = list(outputImagePaths)

        def write(stream_frame, path):
            stream = stream_frame.reshape(-1)[: finalW * finalH]
            if stream.size < finalW * finalH:
                stream = np.concatenate([stream, np.full(finalW * finalH - stream.size, 0xFFFF00FF, dtype=np.uint32)])
            ImageProcessorModel.writeImage(Image(stream.reshape(finalH, finalW).copy()), path, compression=compression)

        with FramePipeline(top.plan(), depth) as pipe:
            done = 0
            for path in inputImagePaths:
                if pipe.pending == depth:
                    write(pipe.collect()[1], todo[done]); done += 1
                # decode straight into the pinned staging buffer (a size mismatch raises IllegalArgumentException)
                ImageProcessorModel.readImageInto(path, pipe.acquire_input())
                pipe.submit()
            while pipe.pending:
                write(pipe.collect()[1], todo[done]); done += 1


def _order_tag(step: ProcessingStep) -> str:
    # `${op.toString.split('.').last.take(2)}` on a ChiselEnum value "ProcessingStep(1=SpatialSampling)"
    # yields "Pr" for every step (ImageCompressorTopApp.scala:188).
    return f"ProcessingStep({int(step)}={step.name})".split(".")[-1][:2]


def _args_map(args: List[str]) -> Dict[str, str]:
    argsMap: Dict[str, str] = {}
    for i in range(0, len(args) - 1, 2):                              # args.sliding(2, 2), :149-151
        if args[i].startswith("--"):
            argsMap[args[i]] = args[i + 1]
    return argsMap


DECOMPRESS_HELP = """usage: python -m csic_amd.app decompress --input x.csic (--output x.png [--frame K] | --output-pattern frame_%03d.png)
                                         [--window x,y,w,h] [--scale s]
  --input           a .csic container of any version
  --output          the PNG to write: frame 0, or frame K with --frame K
  --output-pattern  a printf pattern: every frame of the container is written
  --window x,y,w,h  decode only this rectangle of the frame, given in source pixels (default: the whole frame); a window outside
                    the frame is refused
  --scale s         reduce by an s x s box, s = 1, 2, 4, 8 or 16 (default 1): each output pixel is the rounded mean of the s x s
                    decoded pixels under it.  The PNG is (w // s) x (h // s) pixels: the remainder of a window that is no multiple
                    of s is dropped at its right and bottom edges; a window smaller than one box is refused
Without --window and --scale the whole frame is decoded at its original size."""


def _main_container(verb: str, args: List[str]) -> int:
    """`compress` / `decompress`: the keys of the verb-less CLI with its defaults, plus --output and (compress) --sampling avg and
    --coding raw|groups|rice|rans."""
    rows = verb == "compress" and "--rows" in args          # a flag without a value: taken out before the pairs are read
    argsMap = _args_map([a for a in args if not (rows and a == "--rows")])
    if rows and ("--inputs" in argsMap or "--gop" in argsMap or "--motion" in argsMap or "--target-bytes" in argsMap):
        print("[ERROR] --rows takes one image (--input) and a coding: it does not combine with --inputs, --gop, --motion or --target-bytes")
        return 2
    if verb == "compress" and "--inputs" in argsMap:
        if "--target-bytes" in argsMap:
            print("[ERROR] --target-bytes takes one image (--input): sequences under a byte budget are not supported")
            return 2
        return _main_sequence(argsMap)
    window, scale = None, 1
    if verb == "decompress":
        if "--help" in args:
            print(DECOMPRESS_HELP)
            return 0
        try:
            scale = int(argsMap.get("--scale", "1"))
        except ValueError:
            scale = 0
        if "--window" in argsMap:
            try:
                window = tuple(int(x) for x in argsMap["--window"].split(","))
            except ValueError:
                window = ()
        if scale not in (1, 2, 4, 8, 16):
            print(f"[ERROR] --scale must be 1, 2, 4, 8 or 16, got {argsMap.get('--scale')}")
            return 2
        if window is not None and len(window) != 4:
            print(f"[ERROR] --window must be x,y,w,h in source pixels, got {argsMap.get('--window')}")
            return 2
    if verb == "decompress" and "--output-pattern" in argsMap and "--input" in argsMap:
        if not os.path.exists(argsMap["--input"]):
            print(f"[ERROR] Input not found: {argsMap['--input']}")
            return 1
        try:
            paths = ImageCompressionApp.decompressImages(argsMap["--input"], argsMap["--output-pattern"], window=window, scale=scale)
        except N.IllegalArgumentException as e:
            print(f"[ERROR] {e}")
            return 1
        print(f"Decompression complete. {len(paths)} frames saved to: {argsMap['--output-pattern']}")
        return 0
    if "--input" not in argsMap or "--output" not in argsMap:
        print(f"[ERROR] {verb} needs --input and --output")
        return 2
    inputPath, outputPath = argsMap["--input"], argsMap["--output"]
    if not os.path.exists(inputPath):
        print(f"[ERROR] Input not found: {inputPath}")
        return 1
    if verb == "decompress":
        if window is None and scale == 1:
            ImageCompressionApp.decompressImage(inputPath, outputPath, frame=int(argsMap.get("--frame", "0")))
        else:
            try:
                ImageCompressionApp.decompressImage(inputPath, outputPath, frame=int(argsMap.get("--frame", "0")), window=window, scale=scale)
            except N.IllegalArgumentException as e:
                print(f"[ERROR] {e}")
                return 1
        print(f"Decompression complete. Output saved to: {outputPath}")
        return 0
    sampling = Sampling.AVG if argsMap.get("--sampling", "hold").lower() == "avg" else Sampling.HOLD_DECIMATE
    coding = argsMap.get("--coding", "raw").lower()
    if coding not in ("raw", "groups", "rice", "rans"):
        print(f"[ERROR] --coding must be rans, raw, groups or rice, got {coding}")
        return 2
    if rows and coding == "raw":
        print("[ERROR] --rows needs --coding rans, groups or rice: the layer gains nothing without a coder")
        return 2
    if "--target-bytes" in argsMap:
        return _main_target(argsMap, inputPath, outputPath, sampling)
    size = ImageCompressionApp.compressImage(
        inputPath, outputPath, int(argsMap.get("--a", "4")), int(argsMap.get("--b", "4")), int(argsMap.get("--yq", "8")),
        int(argsMap.get("--cbq", "8")), int(argsMap.get("--crq", "8")), int(argsMap.get("--sf", "8")),
        ProcessingStep.parse(argsMap.get("--op1", "spatial")), ProcessingStep.parse(argsMap.get("--op2", "color")),
        ProcessingStep.parse(argsMap.get("--op3", "chroma")), sampling, coding=coding, rows=rows)
    print(f"Compression complete. {os.path.getsize(inputPath)} -> {size} bytes. Output saved to: {outputPath}")
    return 0


def _main_target(argsMap: Dict[str, str], inputPath: str, outputPath: str, sampling: Sampling) -> int:
    """`compress --input x.png --output x.csic --target-bytes N [--coding raw|groups|rice|rans]`: --yq / --cbq / --crq are upper bounds."""
    coding = argsMap.get("--coding", "rans").lower()
    if coding not in ("raw", "groups", "rice", "rans"):
        print(f"[ERROR] --coding must be rans, raw, groups or rice, got {coding}")
        return 2
    try:
        target = int(argsMap["--target-bytes"])
    except ValueError:
        print(f"[ERROR] --target-bytes must be a number of bytes, got {argsMap['--target-bytes']}")
        return 2
    if target < 80:
        print(f"[ERROR] --target-bytes must be at least the 80 bytes of a header, got {target}")
        return 2
    try:
        got = ImageCompressionApp.compressImageToSize(
            inputPath, outputPath, int(argsMap.get("--a", "4")), int(argsMap.get("--b", "4")), int(argsMap.get("--yq", "8")),
            int(argsMap.get("--cbq", "8")), int(argsMap.get("--crq", "8")), int(argsMap.get("--sf", "8")),
            ProcessingStep.parse(argsMap.get("--op1", "spatial")), ProcessingStep.parse(argsMap.get("--op2", "color")),
            ProcessingStep.parse(argsMap.get("--op3", "chroma")), sampling, targetBytes=target, coding=coding)
    except (N.IllegalArgumentException, N.CsicRuntimeError) as e:
        if isinstance(e, N.CsicRuntimeError) and e.status != N.EINVAL_SIZE:
            raise
        print(f"[ERROR] {e}")
        return 1
    y, cb, cr = got["bits"]
    print(f"Compression complete. Bits Y/Cb/Cr {y}/{cb}/{cr}, estimated {got['est_bytes']} bytes, written {got['bytes']} bytes "
          f"(target {target}) in {got['tries']} tries. PSNR Y/Cb/Cr {got['psnr'][0]:.2f}/{got['psnr'][1]:.2f}/{got['psnr'][2]:.2f} dB. "
          f"Output saved to: {outputPath}")
    return 0


def _main_sequence(argsMap: Dict[str, str]) -> int:
    """`compress --inputs a.png,b.png,... --gop K --coding groups|rice|rans --output x.csic`: frames of equal size as one version-5 container (--motion: 6; rans: 7)."""
    if "--output" not in argsMap:
        print("[ERROR] compress needs --inputs and --output")
        return 2
    paths = [p for p in argsMap["--inputs"].split(",") if p]
    for p in paths:
        if not os.path.exists(p):
            print(f"[ERROR] Input not found: {p}")
            return 1
    coding = argsMap.get("--coding", "rice").lower()
    if coding not in ("groups", "rice", "rans") or not paths:
        print(f"[ERROR] a sequence needs at least one input and --coding rans, groups or rice, got {coding}")
        return 2
    sampling = Sampling.AVG if argsMap.get("--sampling", "hold").lower() == "avg" else Sampling.HOLD_DECIMATE
    size = ImageCompressionApp.compressSequence(
        paths, argsMap["--output"], int(argsMap.get("--a", "4")), int(argsMap.get("--b", "4")), int(argsMap.get("--yq", "8")),
        int(argsMap.get("--cbq", "8")), int(argsMap.get("--crq", "8")), int(argsMap.get("--sf", "8")),
        ProcessingStep.parse(argsMap.get("--op1", "spatial")), ProcessingStep.parse(argsMap.get("--op2", "color")),
        ProcessingStep.parse(argsMap.get("--op3", "chroma")), sampling, coding=coding, gop=int(argsMap.get("--gop", "16")),
        motion=int(argsMap["--motion"]) if "--motion" in argsMap else None)
    print(f"Compression complete. {len(paths)} frames, {sum(os.path.getsize(p) for p in paths)} -> {size} bytes. Output saved to: {argsMap['--output']}")
    return 0


def _vector_of(s: int, w: int, R: int) -> str:
    """The candidate a table word stands for: the (dy, dx) of [-R, R]^2 with dy * w + dx == s that has the lowest rank -- by
    (|dx| + |dy|, dy, dx), the encoder's order; in narrow planes several have the same offset -- or the bare offset if there is none
    (a file not written by this encoder)."""
    hits = [(abs(dx) + abs(dy), dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if dy * w + dx == s]
    return f"({min(hits)[1]}, {min(hits)[2]})" if hits else f"offset {s}"


def _main_inspect(args: List[str]) -> int:
    """`inspect`: the header needs no GPU, the statistics do; without a device the header is printed, then the library's message."""
    argsMap = _args_map(args)
    if "--input" not in argsMap:
        print("[ERROR] inspect needs --input")
        return 2
    inputPath = argsMap["--input"]
    if not os.path.exists(inputPath):
        print(f"[ERROR] Input not found: {inputPath}")
        return 1
    info = container_info(inputPath)
    p = info.params
    ops = " -> ".join(ProcessingStep(int(o)).name for o in p.op)
    print(f"Container: {inputPath} (version {info.version}, {info.file_bytes} bytes)")
    print(f"Image: {p.width}x{p.height}, chroma 4:{p.chroma_a}:{p.chroma_b}, bits Y/Cb/Cr {p.y_bits}/{p.cb_bits}/{p.cr_bits}, "
          f"factor {p.factor}, order {ops}, rounding {p.rounding}, sampling {p.sampling}")
    print(f"Frames: {info.nframes}, payload bytes per frame: {info.payload_bytes}")
    if info.version == 5:
        print(f"Frame coding: {({1: 'groups', 3: 'rice'}).get(info.coding, 'raw')}, temporal delta with gop {info.gop}")
        groups = [max(int(g), 1) for g in delta_layout(p).groups]
        inter = container_inter_groups(inputPath)
        for k, stored in enumerate(container_coded_sizes(inputPath)):
            share = ", ".join(f"{name} {int(inter[k][i]) / groups[i]:.3f}" for i, name in enumerate(("Y", "Cb", "Cr")))
            print(f"  frame {k} ({'key' if k % info.gop == 0 else 'delta'}): stored in {int(stored)} bytes, {int(stored) / info.payload_bytes:.4f} of raw, "
                  f"inter groups {share}")
    elif info.version == 6:
        print(f"Frame coding: {({1: 'groups', 3: 'rice'}).get(info.coding, 'raw')}, motion-compensated delta with gop {info.gop}, range {info.motion}")
        ml = mc_layout(p)
        sizes = container_coded_sizes(inputPath)
        with open(inputPath, "rb") as fh:
            at = 88 + 8 * info.nframes
            for k, stored in enumerate(sizes):
                print(f"  frame {k} ({'key' if k % info.gop == 0 else 'delta'}): stored in {int(stored)} bytes, {int(stored) / info.payload_bytes:.4f} of raw")
                if k % info.gop:
                    fh.seek(at)
                    m = np.frombuffer(fh.read(ml.map_bytes), dtype=np.uint8)
                    for i, name in enumerate(("Y", "Cb", "Cr")):
                        words = m[ml.table_offset[i]:ml.table_offset[i] + 64].view("<i4")
                        sec = m[ml.map_offset[i]:ml.map_offset[i] + (ml.groups[i] + 1) // 2]
                        nib = np.stack([sec & 15, sec >> 4], axis=1).reshape(-1)[:ml.groups[i]]
                        w, G = int(ml.width[i]), max(int(ml.groups[i]), 1)
                        cells = [f"intra {np.count_nonzero(nib == 0) / G:.3f}"]
                        for t in range(1, int(words[0]) + 1):
                            cells.append(f"{_vector_of(int(words[t]), w, info.motion)} {np.count_nonzero(nib == t) / G:.3f}")
                        print(f"    {name} table: " + ", ".join(cells))
                at += int(stored)
    elif info.version == 7:
        with open(inputPath, "rb") as fh:
            fh.seek(84)
            gop = int.from_bytes(fh.read(4), "little")         # 0: every frame stands alone
            layer = "" if gop == 0 else f", temporal delta with gop {gop}" if info.motion < 0 else f", motion-compensated delta with gop {gop}, range {info.motion}"
            print(f"Frame coding: rans{layer}")
            sizes = container_coded_sizes(inputPath)
            for k, stored in enumerate(sizes):
                kind = "" if gop == 0 else " (key)" if k % gop == 0 else " (delta)"
                print(f"  frame {k}{kind}: stored in {int(stored)} bytes, {int(stored) / info.payload_bytes:.4f} of raw")
            rl = rans_layout(p)                                 # frame 0 is a key frame: its record is its coded frame
            fh.seek(88 + 8 * info.nframes + rl.directory_offset)
            directory = np.frombuffer(fh.read(4 * (sum(rl.blocks) + 1)), dtype="<u4")
            for i, name in enumerate(("Y", "Cb", "Cr")):
                b0 = sum(rl.blocks[:i])
                print(f"    frame 0, {name}: {int(np.count_nonzero(directory[b0:b0 + rl.blocks[i]] >> 31))} of {rl.blocks[i]} blocks raw")
    elif info.version == 8:
        print(f"Frame coding: {({1: 'groups', 3: 'rice', 5: 'rans'})[info.coding]}, row prediction (bands of {N.ROWS_BAND} steps)")
        groups = [int(g) for g in rows_layout(p).groups]
        above = container_inter_groups(inputPath)
        for k, stored in enumerate(container_coded_sizes(inputPath)):
            print(f"  frame {k}: stored in {int(stored)} bytes, {int(stored) / info.payload_bytes:.4f} of raw")
            for i, name in enumerate(("Y", "Cb", "Cr")):
                print(f"    frame {k}, {name}: {int(above[k][i])} of {groups[i]} groups ({100.0 * int(above[k][i]) / max(groups[i], 1):.1f}%) predicted from the row above")
    else:
        print(f"Frame coding: {({3: 'groups', 4: 'rice'}).get(info.version, 'raw')}")
        for k, stored in enumerate(container_coded_sizes(inputPath)):
            print(f"  frame {k}: stored in {int(stored)} bytes, {int(stored) / info.payload_bytes:.4f} of raw")
    try:
        c_params, nframes, frames = read_container(inputPath)
        with Plan(c_params, 0) as plan:
            stats = plan.code_stats(frames, N.FMT_PLANAR_BITS, nframes)
    except N.CsicRuntimeError as e:
        if e.status != N.ENODEVICE:
            raise
        print(f"[ERROR] No code statistics: {e}")
        return 0
    for k, st in enumerate(stats if nframes > 1 else [stats]):
        print(f"Frame {k}:")
        for i, name in enumerate(st.PLANES):
            print(f"  {name:<2}: {st.samples[i]} samples, q = {st.bits[i]}, H0 = {st.entropy(0, i):.4f}, H1 = {st.entropy(1, i):.4f} bits / sample")
        raw_bytes = (sum(n * q for n, q in zip(st.samples, st.bits)) + 7) // 8
        print(f"  raw            : {st.raw_bits_per_pixel:.4f} bits / px, {raw_bytes} bytes")
        for label, kind in (("order-0", 0), ("left-predicted", 1), ("best", "best")):
            print(f"  {label:<15}: {st.bits_per_pixel(kind):.4f} bits / px, {st.ideal_bytes(kind)} bytes")
    return 0


def main(argv: List[str] = None) -> int:
    args = list(sys.argv[1:] if argv is None else argv)
    if args and args[0] == "inspect":
        return _main_inspect(args[1:])
    if args and args[0] in ("compress", "decompress"):
        return _main_container(args[0], args[1:])
    argsMap = _args_map(args)
    inputPath = argsMap.get("--input", "test_images/in128x128.png")
    a = int(argsMap.get("--a", "4"))
    b = int(argsMap.get("--b", "4"))
    yq = int(argsMap.get("--yq", "8"))
    cbq = int(argsMap.get("--cbq", "8"))
    crq = int(argsMap.get("--crq", "8"))
    sf = int(argsMap.get("--sf", "8"))
    op1 = ProcessingStep.parse(argsMap.get("--op1", "spatial"))
    op2 = ProcessingStep.parse(argsMap.get("--op2", "color"))
    op3 = ProcessingStep.parse(argsMap.get("--op3", "chroma"))
    imageName = os.path.basename(inputPath).split(".")[0]

    print("----------------------------------------------------")
    print("Image Compressor Application Parameters:")
    print("----------------------------------------------------")
    print(f"Input Image: {inputPath}")
    print(f"Selected Chroma Subsampling (J:a:b): 4:{a}:{b}")
    print(f"Selected Quantization Bits (Y/Cb/Cr): {yq}/{cbq}/{crq}")
    print(f"Selected Spatial Downsampling Factor: {sf}")
    print(f"Selected Pipeline Order: {op1.name} -> {op2.name} -> {op3.name}")
    print("----------------------------------------------------")

    outDir = argsMap.get("--outdir", "APP_OUTPUT")
    order = f"order-{_order_tag(op1)}-{_order_tag(op2)}-{_order_tag(op3)}"
    suffix = f"chroma4-{a}-{b}_Y{yq}Cb{cbq}Cr{crq}_sf{sf}_{order}"
    outputPath = f"{outDir}/{imageName}_processed_{suffix}.png"
    os.makedirs(outDir, exist_ok=True)
    if not os.path.exists(inputPath):
        print(f"[ERROR] Input image not found: {inputPath}")          # :197-199 (not an exception)
        return 0
    # not a key of the reference's CLI: `--collector-budget emulate` reproduces its collector's cycle budget (see processImage)
    emulate = argsMap.get("--collector-budget", "off") == "emulate"
    ImageCompressionApp.processImage(inputPath, outputPath, a, b, yq, cbq, crq, sf, op1, op2, op3, emulateCollectorBudget=emulate)
    print(f"Image processing complete. Output saved to: {outputPath}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
