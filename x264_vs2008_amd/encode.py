"""The reference's command line for what this library builds: raw I420 / YUV4MPEG2 in, Annex B `.264` out, on the GPU.

    python -m x264_vs2008_amd.encode --crf 23 --ref 3 --bframes 3 --b-adapt 1 --subme 7 --8x8dct --trellis 1 --weightb --mixed-refs -o out.264 in.y4m
    python -m x264_vs2008_amd.encode --qp 26 --no-cabac --me dia --subme 0 --partitions none --no-deblock --scenecut -1 -o out.264 in.yuv 352x288
    python -m x264_vs2008_amd.encode --crf 23 --no-cabac --subme 5 --bframes 2 -o out.264 in.y4m      # CAVLC through the frame queue: CRF, B frames, scene cuts
    python -m x264_vs2008_amd.encode [options] -o out_%d.264 a.y4m b.y4m c.y4m        # one stream per input, coded side by side (same size and options)
    python -m x264_vs2008_amd.encode --input-csp nv12 --qp 26 -o out.264 in_352x288.nv12                  # raw NV12 (Y plane, interleaved UV plane); also yv12, and --vflip
    python -m x264_vs2008_amd.encode --qp 0 -o out.264 in.y4m                         # lossless (High 4:4:4 Predictive SPS): what x264_validate_parameters
                                                                                      # turns off at QP 0 is off here too, the lookahead scores with SAD

Option names and meanings are `x264 --longhelp`'s (R/x264.c:386-487, x264_param_parse R/common/common.c:206-587; tests/test_cpu_encode_cli.py
parses the same argument lists with the reference's own x264_param_parse and compares x264_param2string).  The parameters go through
x264hip_validate_parameters (what x264_encoder_open does to them), the encoder runs with the validated values, and the output is what
x264_encoder_encode emits: version SEI, SPS, PPS, one slice NAL per frame in coding order (x264_vs2008_amd/mux.py).  For BASELINE's flag
sets the file is the reference command line's, byte for byte (tests/test_gpu_encode_cli.py).

A single stream is one serial chain of macroblocks -- ONE wavefront: a lone 1080p input codes at well under a frame per second.  The
product's throughput comes from thousands of streams in flight (bench.py); this front end is the functional drop-in, and several inputs
given at once are coded as chains of one batch.

Readers: raw I420 (R/muxers.c:63-122: frame i at i * w * h * 3 / 2) and YUV4MPEG2 (:124-316: W, H, F from the stream header, C420* only, every
FRAME header skipped to its newline).  Not the reference's: --input-csp yv12 / nv12 and --vflip say how a raw file's frames are laid out (x264_picture_t.img.i_csp
has I420, YV12 and X264_CSP_VFLIP, its command line no option for them); such frames are not rearranged on the host -- every stream's frame is read into one
pinned block, goes to the device in one copy and becomes the encoder's picture in one launch (x264hip_picture_import).  Refused, never approximated: what the library refuses (x264hip_validate_parameters, the encoders' own
checks) -- ABR / VBV / 2-pass, --direct none, --no-cabac with --subme 6 and above (the RD levels), interlaced, threads > 1, b-pyramid.
Every coded frame is measured as x264 does by default (PSNR, SSIM, macroblock statistics: --no-psnr / --no-ssim / --quiet turn that off, -v prints
x264_encoder_frame_end's line per frame) and x264_encoder_close's report goes to stderr at the end, one per stream; the `.264` bytes do not depend on it.
Scene cuts work as in the reference: by default after the fact (a P picture that should have been intra is coded again, encoder.c:1603-1699), with
--pre-scenecut in the lookahead.  --nr N goes with all of it -- B frames, adaptive B placement, --direct auto, --no-cabac, the RD levels, trellis,
adaptive quantisation and either scene cut: x264_noise_reduction_update runs once per returned frame of a stream, behind a given-up attempt's second
encode as in the reference (stream.py: _nr_update).  Lossless turns it off, as x264_validate_parameters does."""
import argparse
import os
import re
import sys
import time

import numpy as np

from . import mux
from .frame import CSP_I420, CSP_NV12, CSP_VFLIP, CSP_YV12

ME = {"dia": 0, "hex": 1, "umh": 2, "esa": 3, "tesa": 4}
DIRECT = {"none": 0, "spatial": 1, "temporal": 2, "auto": 3}
CQM = {"flat": 0, "jvt": 1}
INPUT_CSP = {"i420": CSP_I420, "yv12": CSP_YV12, "nv12": CSP_NV12}


def build_parser():
    ap = argparse.ArgumentParser(prog="x264_vs2008_amd.encode", description="x264 core 66's command line on MI355X (the built subset)", allow_abbrev=False)
    a = ap.add_argument
    a("inputs", nargs="+", help="raw I420 (.yuv, with WxH as the last argument or in the name) or YUV4MPEG2 (.y4m) files; several inputs = several streams side by side")
    a("-o", "--output", required=True, help="output .264; with several inputs a pattern with %%d")
    a("--frames", type=int, default=0, help="maximum number of frames to encode")
    a("--fps", default=None, help="float or rational (raw input; y4m carries its own)")
    a("-q", "--qp", type=int, default=None, help="constant quantiser")
    a("--crf", type=float, default=None, help="quality-based VBR (nominal QP)")
    a("-r", "--ref", type=int, default=1)
    a("-b", "--bframes", type=int, default=0)
    a("--b-adapt", type=int, default=1)
    a("--b-bias", type=int, default=0)
    a("-I", "--keyint", type=int, default=250)
    a("-i", "--min-keyint", type=int, default=25)
    a("--scenecut", type=int, default=40)
    a("--pre-scenecut", action="store_true")
    a("--no-cabac", action="store_true")
    a("--cavlc-mp", action="store_true", help="with --no-cabac: write the slices with the macroblock-parallel CAVLC pass (same bytes)")
    a("--no-deblock", "--nf", action="store_true")
    a("-f", "--deblock", default=None, help="alpha:beta (negative alpha: write --deblock=-1:2)")
    a("-A", "--partitions", "--analyse", default=None, help="p8x8,p4x4,b8x8,i8x8,i4x4 / none / all")
    a("--direct", default="spatial", choices=sorted(DIRECT))
    a("-w", "--weightb", action="store_true")
    a("--me", default="hex", choices=sorted(ME))
    a("--merange", type=int, default=16)
    a("--mvrange", type=int, default=-1)
    a("-m", "--subme", type=int, default=6)
    a("--psy-rd", default="1.0:0.0", help="rd:trellis strengths")
    a("--mixed-refs", action="store_true")
    a("--no-chroma-me", action="store_true")
    a("--8x8dct", dest="dct8", action="store_true")       # (no -8: a digit option would make argparse read "--scenecut -1" as two options)
    a("-t", "--trellis", type=int, default=0)
    a("--no-fast-pskip", action="store_true")
    a("--no-dct-decimate", action="store_true")
    a("--nr", type=int, default=0)
    a("--deadzone-inter", type=int, default=21)
    a("--deadzone-intra", type=int, default=11)
    a("--cqm", default="flat", choices=sorted(CQM))
    a("--chroma-qp-offset", type=int, default=0)
    a("--ipratio", type=float, default=1.4)
    a("--pbratio", type=float, default=1.3)
    a("--qcomp", type=float, default=0.6)
    a("--qpmin", type=int, default=10)
    a("--qpmax", type=int, default=51)
    a("--qpstep", type=int, default=4)
    a("--aq-mode", type=int, default=1)
    a("--aq-strength", type=float, default=1.0)
    a("--level", default=None, help="4.1 / 41 ...")
    a("--threads", type=int, default=1)
    a("--no-asm", action="store_true", help="accepted and ignored (there is no asm here)")
    a("--no-psnr", action="store_true", help="disable PSNR computation")
    a("--no-ssim", action="store_true", help="disable SSIM computation")
    a("--quiet", action="store_true", help="quiet mode: no statistics (a log level below INFO turns both measurements off, R/encoder/encoder.c:587-591)")
    a("-v", "--verbose", action="store_true", help="print stats for each frame")
    a("--device", type=int, default=0, help="GPU to run on")
    a("--input-csp", default="i420", choices=sorted(INPUT_CSP), help="layout of raw input frames: i420 (Y, U, V), yv12 (Y, V, U), nv12 (Y, interleaved UV)")
    a("--vflip", action="store_true", help="raw input frames are stored bottom-up")
    return ap


def param_fields(o):
    """The command line as x264_param_t fields (x264hip_encoder_params' names): what x264_param_parse does with each option."""
    k = dict(frame_reference=o.ref, bframe=o.bframes, bframe_adaptive=o.b_adapt, bframe_bias=o.b_bias, keyint_max=o.keyint, keyint_min=o.min_keyint,
             scenecut_threshold=o.scenecut, pre_scenecut=int(o.pre_scenecut), cabac=int(not o.no_cabac), deblocking_filter=int(not o.no_deblock),
             direct_mv_pred=DIRECT[o.direct], weighted_bipred=int(o.weightb), me_method=ME[o.me], me_range=o.merange, mv_range=o.mvrange, subpel_refine=o.subme,
             mixed_references=int(o.mixed_refs), chroma_me=int(not o.no_chroma_me), transform_8x8=int(o.dct8), trellis=o.trellis, fast_pskip=int(not o.no_fast_pskip),
             dct_decimate=int(not o.no_dct_decimate), noise_reduction=o.nr, luma_deadzone=(o.deadzone_inter, o.deadzone_intra), cqm_preset=CQM[o.cqm],
             chroma_qp_offset=o.chroma_qp_offset, ip_factor=o.ipratio, pb_factor=o.pbratio, qcompress=o.qcomp, qp_min=o.qpmin, qp_max=o.qpmax, qp_step=o.qpstep,
             aq_mode=o.aq_mode, aq_strength=o.aq_strength, threads=o.threads)
    if o.deblock is not None:                      # "deblock" / "filter": alpha[:beta], a lone number gives both (common.c:336-347)
        parts = re.split("[:,]", o.deblock)
        k["deblocking_filter_alphac0"] = int(parts[0])
        k["deblocking_filter_beta"] = int(parts[1]) if len(parts) > 1 else int(parts[0])
        k["deblocking_filter"] = 1
    pr = re.split("[:,]", o.psy_rd)
    k["psy_rd"] = float(pr[0])
    k["psy_trellis"] = float(pr[1]) if len(pr) > 1 else 0.0
    if o.partitions is not None:                   # common.c:398-418: the option rewrites analyse.inter only
        v, inter = o.partitions, 0
        if "all" in v:
            inter = 0xffffffff                     # ~0; x264_validate_parameters masks it
        for name, bit in (("i4x4", 0x1), ("i8x8", 0x2), ("p8x8", 0x10), ("p4x4", 0x20), ("b8x8", 0x100)):
            if name in v:
                inter |= bit
        k["inter"] = inter
    if o.qp is not None:                           # common.c:446-451 / 440-445: the last of --qp / --crf given wins; both given: CRF here as in the usual order
        k.update(rc_method=mux.RC_CQP, qp_constant=o.qp)
    if o.crf is not None:
        k.update(rc_method=mux.RC_CRF, rf_constant=o.crf)
    if o.level is not None:                        # common.c:262-268: "4.1" -> 41, small integers are tenths
        lv = o.level
        k["level_idc"] = int(10 * float(lv) + .5) if "." in lv or int(lv) < 6 else int(lv)
    return k


def report_fields(o):
    """param.analyse.b_psnr / b_ssim and the log level as the command line leaves them: both measurements are x264's defaults (R/common/common.c:131-132),
    --no-psnr / --no-ssim turn one off, --quiet (X264_LOG_NONE) both and the report with them; -v (X264_LOG_DEBUG) adds the per-frame line."""
    return dict(psnr=int(not o.no_psnr and not o.quiet), ssim=int(not o.no_ssim and not o.quiet), verbose=bool(o.verbose and not o.quiet), quiet=bool(o.quiet))


# ---- readers (R/muxers.c) ----------------------------------------------------------------------------------------------------------------
class RawYuv:
    def __init__(self, path, w, h):
        self.f, self.w, self.h = open(path, "rb"), w, h
        self.size = w * h * 3 // 2
        self.n = os.path.getsize(path) // self.size
        self.fps = None

    def read(self, i):
        self.f.seek(i * self.size)
        b = np.frombuffer(self.f.read(self.size), np.uint8)
        if b.size != self.size:
            raise IOError("short read at frame %d" % i)
        w, h = self.w, self.h
        return b[:w * h].reshape(h, w), b[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), b[w * h * 5 // 4:].reshape(h // 2, w // 2)

    def read_into(self, i, out):
        """Frame i as the file holds it, into the uint8 array `out` (self.size bytes)."""
        self.f.seek(i * self.size)
        if self.f.readinto(out) != self.size:
            raise IOError("short read at frame %d" % i)


class Y4m:
    def __init__(self, path):
        self.f = open(path, "rb")
        head = self.f.readline(96)
        if not head.startswith(b"YUV4MPEG2") or not head.endswith(b"\n"):
            raise ValueError("%s: not a YUV4MPEG2 stream" % path)
        self.w = self.h = 0
        self.fps = None
        for tok in head[10:].split():
            t, v = chr(tok[0]), tok[1:].decode()
            if t == "W":
                self.w = int(v)
            elif t == "H":
                self.h = int(v)
            elif t == "C" and not v.startswith("420"):
                raise ValueError("%s: colorspace %s unhandled (4:2:0 only)" % (path, v))
            elif t == "F":
                n, d = (int(x) for x in v.split(":"))
                if n and d:
                    self.fps = (n, d)
        self.seq_len = len(head)
        self.size = self.w * self.h * 3 // 2
        self.offsets, pos, total = [], self.seq_len, os.path.getsize(path)
        while pos < total:                         # every FRAME header may carry parameters: skip to its newline
            self.f.seek(pos)
            fh = self.f.readline(96)
            if not fh.startswith(b"FRAME") or not fh.endswith(b"\n") or pos + len(fh) + self.size > total:
                break
            self.offsets.append(pos + len(fh))
            pos += len(fh) + self.size
        self.n = len(self.offsets)

    def read(self, i):
        self.f.seek(self.offsets[i])
        b = np.frombuffer(self.f.read(self.size), np.uint8)
        w, h = self.w, self.h
        return b[:w * h].reshape(h, w), b[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), b[w * h * 5 // 4:].reshape(h // 2, w // 2)


class DeviceIngest:
    """Input frames in a layout other than top-down I420: frame t of every source is read into ONE pinned block as the file holds it, copied
    to ONE device buffer in one copy, and handed to the encoder as surfaces for one x264hip_picture_import -- the layout is undone by the
    kernel, not on the host."""

    def __init__(self, lib, sources, csp, vflip):
        import ctypes as C
        self.lib, self.sources, self.size = lib, sources, sources[0].size
        w, h = sources[0].w, sources[0].h
        if not all(hasattr(s, "read_into") for s in sources):
            raise ValueError("--input-csp / --vflip go with raw input: a YUV4MPEG2 stream names its own layout")
        if w % 2 or h % 2:
            raise ValueError("--input-csp / --vflip: %dx%d: 4:2:0 surfaces have even sizes" % (w, h))
        n = self.size * len(sources)
        self.host = lib.x264hip_host_alloc(n)
        self.dev = lib.x264hip_malloc(n)
        self.ev = lib.x264hip_event_create()
        if not self.host or not self.dev or not self.ev:
            self.close()
            raise MemoryError("--input-csp / --vflip: %d bytes of pinned and device memory" % n)
        self.view = np.ctypeslib.as_array(C.cast(self.host, C.POINTER(C.c_uint8)), (len(sources), self.size))
        self.busy = False
        flags = csp | (CSP_VFLIP if vflip else 0)
        if csp == INPUT_CSP["nv12"]:
            self.layout = lambda base: (flags, (base, base + w * h, None), (w, w, 0))
        else:                                      # the second and third plane as the file orders them: YV12 is the layout's name for V first
            self.layout = lambda base: (flags, (base, base + w * h, base + w * h * 5 // 4), (w, w // 2, w // 2))

    def surfaces(self, t, stream):
        """Frame t of every source on the device, behind what `stream` holds: the entries for FrameCtx.import_surfaces on that stream."""
        lib = self.lib
        if self.busy and lib.x264hip_event_query(self.ev) != 1:        # the copy of the frame before still reads the pinned block
            lib.x264hip_stream_synchronize(stream)
        for b, s in enumerate(self.sources):
            s.read_into(t, self.view[b])
        if lib.x264hip_memcpy_h2d_async(self.dev, self.host, self.view.size, stream) != 0 or lib.x264hip_event_record(self.ev, stream) != 0:
            raise RuntimeError("--input-csp / --vflip: frame %d to the device: %s" % (t, lib.x264hip_last_error().decode()))
        self.busy = True
        return [(b,) + self.layout(self.dev + b * self.size) for b in range(len(self.sources))]

    def close(self):
        if self.ev:
            self.lib.x264hip_event_destroy(self.ev)
        if self.dev:
            self.lib.x264hip_free(self.dev)
        if self.host:
            self.lib.x264hip_host_free(self.host)
        self.ev = self.dev = self.host = self.view = None


def open_inputs(names):
    """The command line's file arguments: inputs, with `WxH` as an optional last argument for raw files (or WxH in a raw file's name)."""
    names = list(names)
    res = None
    if len(names) > 1 and re.fullmatch(r"\d+x\d+", names[-1]):
        res = tuple(int(v) for v in names.pop().split("x"))
    out = []
    for n in names:
        if n.lower().endswith(".y4m"):
            out.append(Y4m(n))
        else:
            r = res
            if r is None:
                m = re.search(r"(\d+)x(\d+)", os.path.basename(n))
                if not m:
                    raise ValueError("%s: raw input needs its resolution (WxH as the last argument or in the file name)" % n)
                r = (int(m.group(1)), int(m.group(2)))
            out.append(RawYuv(n, *r))
    return out


# ---- the encoders -------------------------------------------------------------------------------------------------------------------------
def needs_lookahead(p):
    """x264_encoder_open: h->frames.b_have_lowres (encoder.c:711-716), plus anything that needs the frame queue at all."""
    return bool(p.bframe or p.rc_method == mux.RC_CRF or (p.scenecut_threshold >= 0 and p.keyint_max > 1))


def check_built(p):
    """What the validated parameters p ask for that no encoder here builds, said before anything is allocated.  x264_validate_parameters has
    already done what the reference does for !b_cabac (trellis off); CAVLC slices -- I, P and B, constant QP or CRF, with or without scene
    cuts -- are coded below the RD levels only."""
    if not p.cabac and p.subpel_refine >= 6:
        raise ValueError("--no-cabac with --subme %d: the RD levels price CAVLC bits with a counting twin of the writer, which is not built "
                         "(--subme 5 and below are)" % p.subpel_refine)
    if p.inter & 0x20 and p.subpel_refine >= 6 and p.bframe:
        raise ValueError("--partitions with p4x4 at --subme %d together with --bframes %d: sub-8x8 partitions under the RD levels are built for I / P "
                         "streams (--bframes 0); the B kernels do not keep the cache entries a macroblock leaves behind" % (p.subpel_refine, p.bframe))


def encode_streams(lib, p, sources, n_frames, sinks, psnr=0, ssim=0, verbose=False, stats=None, observe=None, cabac_pass=None, cavlc_mp=None,
                   input_csp=INPUT_CSP["i420"], vflip=False):
    """p: validated parameters (mux.encoder_params); sources: readers of equal picture size; sinks: binary files, one per source.
    psnr / ssim: measure every coded frame (x264hip_frame_report_*); stats: a list that receives one quality.Stat per stream (the caller prints
    its summary and closes it); verbose: x264_encoder_frame_end's line per frame on stderr; observe(enc, chain, frame, slice type, picture, state,
    muxer): called for every accounted frame while its reconstruction and state are still on the device (a checker's view of what was measured).
    cabac_pass: who writes a CABAC slice of a stream without lookahead (constant QP, no B frames, no scene cuts) -- None: the pass behind the
    sweep (ChainEncoder(cabac_pass=True)) below the RD levels, without trellis and adaptive quantisation, not lossless -- where the sweep in
    front of it is the macroblock-parallel one, measured faster; under --aq-mode 1 both choices code a frame on one wavefront
    per chain and nothing has been measured, so the in-loop writer stays; True / False force it either way.  The bytes are the same.
    cavlc_mp: who writes a --no-cabac slice wherever the CAVLC pass runs -- True: the macroblock-parallel pass (ChainEncoder(cavlc_mp=True):
    count, scan, place), None / False: the serial pass; a ValueError where no CAVLC pass runs (CABAC).  The bytes are the same.
    input_csp / vflip: the layout of the sources' frames (INPUT_CSP); anything but top-down I420 goes through DeviceIngest."""
    check_built(p)
    ingest = DeviceIngest(lib, sources, input_csp, vflip) if input_csp != INPUT_CSP["i420"] or vflip else None
    try:
        return _encode_streams(lib, p, sources, n_frames, sinks, psnr, ssim, verbose, stats, observe, cabac_pass, cavlc_mp, ingest)
    finally:
        if ingest is not None:
            ingest.close()


def _encode_streams(lib, p, sources, n_frames, sinks, psnr, ssim, verbose, stats, observe, cabac_pass, cavlc_mp, ingest):
    from .quality import Stat
    if stats is not None:
        stats += [Stat(lib, p, psnr, ssim) for _ in sources]
    measure = dict(psnr=psnr, ssim=ssim, mb_stats=1) if stats is not None else {}
    last_anchor = [None] * len(sources)

    def account(b, record, stype, frame, direct_spatial=1, where=None):
        """x264_encoder_frame_end for stream b's frame, from what its muxer just wrote."""
        m = muxers[b].last
        if observe is not None:
            observe(enc, b, frame, stype, where[0], where[1], muxers[b])
        since = 0 if last_anchor[b] is None else frame - last_anchor[b] - 1
        line = stats[b].frame_end(record, stype, m["frame_size"], nal_ref_idc=m["nal_ref_idc"], poc=m["poc"], frames_since_ref=since, direct_spatial=direct_spatial)
        if stype != sl.SLICE_B:
            last_anchor[b] = frame
        if verbose:
            sys.stderr.write(("%s: " % getattr(sinks[b], "name", b) if len(sources) > 1 else "") + line)
    from .frame import JVT_LISTS, cqm_init
    from . import slice as sl
    B, w, h = len(sources), p.width, p.height
    dz = (p.luma_deadzone[0], p.luma_deadzone[1])
    cq = cqm_init(lib, JVT_LISTS if p.cqm_preset == 1 else None, luma_deadzone=dz, qp_min=p.qp_min)
    muxers = [mux.AnnexB(lib, p) for _ in range(B)]
    common = dict(qp=p.qp_constant, me_method=p.me_method, me_range=p.me_range, subme=p.subpel_refine, n_refs=p.frame_reference, inter=p.inter, intra=p.intra,
                  transform8x8=p.transform_8x8, fast_pskip=p.fast_pskip, dct_decimate=p.dct_decimate, chroma_me=p.chroma_me, cabac=p.cabac, deblock=p.deblocking_filter,
                  alpha_c0=p.deblocking_filter_alphac0, beta=p.deblocking_filter_beta, keyint=p.keyint_max, mixed_refs=p.mixed_references, noise_reduction=p.noise_reduction,
                  mv_range=p.mv_range, trellis=p.trellis, psy_rd=p.psy_rd, psy_trellis=p.psy_trellis, aq_mode=p.aq_mode, aq_strength=p.aq_strength, qp_min=p.qp_min, qp_max=p.qp_max)
    # chroma_qp_offset: the encoders apply the two psy shifts themselves (as x264_validate_parameters did to p): hand them the value before both
    shift = (1 if p.psy_rd < 0.25 else 2) if p.d_psy_rd_fix8 else 0
    if sl.psy_trellis_fix8(p.psy_trellis):     # h->mb.i_psy_trellis (p.psy_trellis is 0 without trellis)
        shift += 1 if p.psy_trellis < 0.25 else 2
    common["chroma_qp_offset"] = p.chroma_qp_offset + shift
    coded = 0
    if not needs_lookahead(p):
        # x264_slicetype_decide has nothing to decide: an IDR every keyint frames, P frames between, constant QP
        if cabac_pass is None:
            cabac_pass = bool(p.cabac and p.subpel_refine < 6 and not p.trellis and not p.aq_mode and p.qp_constant != 0)
        # --partitions all at --subme 6..9: the chain's record of cache leftovers (x264hip_slice_rd.mb_carry); the frame queue's encoder turns it on itself
        carry = bool(p.inter & 0x20 and p.subpel_refine >= 6 and p.qp_constant != 0)
        enc = sl.ChainEncoder(lib, w, h, cq, batch=B, write=1, cabac_pass=cabac_pass or None, mb_carry=carry, cavlc_mp=cavlc_mp, **common, **measure)
        try:
            for t in range(n_frames):
                if ingest is not None:
                    enc.upload_device(ingest.surfaces(t, enc.ctx.stream))
                else:
                    for b, s in enumerate(sources):
                        enc.upload(*s.read(t), b=b)
                stype, qp, _ = enc.encode_frame()
                enc.status()
                pays = enc.payloads()
                enc.finish_frame()
                recs = None
                if stats is not None:
                    enc.sync()
                    recs = enc.reports()
                for b in range(B):
                    sinks[b].write(muxers[b].frame(frame=t, ftype=mux.TYPE_IDR if stype == sl.SLICE_I else mux.TYPE_P, qp=qp, payload=pays[b]))
                    if recs is not None:
                        account(b, recs[b], stype, t, where=enc.last)
                coded += 1
        finally:
            enc.close()
        return coded
    from .stream import StreamEncoder
    enc = StreamEncoder(lib, w, h, cq, batch=B, n_frames=n_frames, crf=p.rf_constant if p.rc_method == mux.RC_CRF else None, b_adapt=p.bframe_adaptive,
                        bframe_bias=p.bframe_bias, keyint_min=p.keyint_min, scenecut_threshold=p.scenecut_threshold, pre_scenecut=p.pre_scenecut,
                        ip_factor=p.ip_factor, pb_factor=p.pb_factor, qcompress=p.qcompress, qp_step=p.qp_step, bframes=p.bframe, weightb=p.weighted_bipred,
                        direct_pred=p.direct_mv_pred, cavlc_mp=cavlc_mp, **common, **measure)

    def fill(pic, f):
        if ingest is not None:
            enc.src_ctx.import_surfaces(pic, ingest.surfaces(f, enc.src_ctx.stream))
            return
        for b, s in enumerate(sources):
            enc.src_ctx.upload(pic, *s.read(f), b=b)

    try:
        idle = 0
        while idle < 2 and coded < n_frames * B:
            out = enc.step(fill)
            idle = 0 if out else idle + bool(enc.flushing)
            if out:
                enc.sync()
                enc.status()
                pays = enc.payloads()
                for cd in out:
                    sinks[cd.chain].write(muxers[cd.chain].frame(frame=cd.frame, ftype=cd.type, qp=cd.qp, payload=pays[cd.chain], n_ref0=cd.n_ref0, n_ref1=cd.n_ref1,
                                                                 direct_spatial=cd.direct_spatial, frame_num_reset=cd.frame_num_reset))
                    if stats is not None:
                        account(cd.chain, enc.report_of(cd), cd.slice_type, cd.frame, cd.direct_spatial, where=(enc.pool[cd.pic], enc.states[cd.pic]))
                    coded += 1
    finally:
        enc.close()
    return coded // B


def main(argv=None):
    o = build_parser().parse_args(argv)
    if (o.input_csp != "i420" or o.vflip) and any(n.lower().endswith(".y4m") for n in o.inputs):
        raise SystemExit("encode: %s goes with raw input: a YUV4MPEG2 stream names its own layout (planar 4:2:0, U before V, top-down)"
                         % ("--vflip" if o.input_csp == "i420" else "--input-csp " + o.input_csp))
    from . import lib as L
    sources = open_inputs(o.inputs)
    w, h = sources[0].w, sources[0].h
    if any((s.w, s.h) != (w, h) for s in sources):
        raise SystemExit("encode: all inputs must have the same picture size")
    n = min(s.n for s in sources)
    if any(s.n != n for s in sources):             # the chains of a batch take their pictures in lock step: every stream ends with the shortest input
        print("encode: inputs of different lengths (%s frames): every stream is coded up to the shortest, %d frames" % (", ".join(str(s.n) for s in sources), n), file=sys.stderr)
    if o.frames > 0:
        n = min(n, o.frames)
    if n < 1:
        raise SystemExit("encode: no frames")
    k = param_fields(o)
    fps = sources[0].fps
    if o.fps is not None:                          # common.c:280-296: "25", "30000/1001", "23.976"
        if "/" in o.fps:
            fps = tuple(int(v) for v in o.fps.split("/"))
        else:
            f = float(o.fps)
            fps = (int(f * 1000 + .5), 1000)
    if fps:
        k.update(fps_num=fps[0], fps_den=fps[1])
    lib = L.load(o.device)
    try:
        p = mux.encoder_params(lib, width=w, height=h, **k)
    except ValueError as ex:
        raise SystemExit("encode: " + str(ex))
    if len(sources) > 1 and "%d" not in o.output:
        raise SystemExit("encode: several inputs need an output pattern with %d")
    names = [o.output % i if "%d" in o.output else o.output for i in range(len(sources))]
    sinks = [open(nm, "wb") for nm in names]
    rf = report_fields(o)
    stats = None if rf["quiet"] else []
    t0 = time.time()
    try:
        done = encode_streams(lib, p, sources, n, sinks, psnr=rf["psnr"], ssim=rf["ssim"], verbose=rf["verbose"], stats=stats, cavlc_mp=o.cavlc_mp or None,
                              input_csp=INPUT_CSP[o.input_csp], vflip=o.vflip)
    except (ValueError, RuntimeError) as ex:
        raise SystemExit("encode: " + str(ex))
    finally:
        for s in sinks:
            s.close()
    dt = max(time.time() - t0, 1e-6)
    # x264_encoder_close's report per stream, then the command line's own last line (R/x264.c:890-897: the file's bytes over the clip's duration)
    for b, st in enumerate(stats or []):
        pre = "%s: " % names[b] if len(sources) > 1 else ""
        sys.stderr.write("".join(pre + ln + "\n" for ln in st.summary().splitlines()))
        sys.stderr.write("%sencoded %d frames, %.2f fps, %.2f kb/s\n" % (pre, done, done / dt, float(os.path.getsize(names[b])) * 8 * p.fps_num / (float(p.fps_den) * done * 1000)))
        st.close()
    print("encoded %d frames of %d stream%s (%dx%d): %s" % (done, len(sources), "" if len(sources) == 1 else "s", w, h, ", ".join(names)), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
