"""Host side of the macroblock sweep (include/x264hip.h: x264hip_slice_sweep_frame; its records -- MbState, SliceParams, SliceRd,
SliceB ... -- are abi.py's) and a chain encoder around it: I frame, then P frames, every frame kept as reference -- the sequencing
x264_encoder_encode / x264_slice_write / x264_fdec_filter_row do on the host
(R/encoder/encoder.c:1316-1560, 1141-1291, 983-1056), restricted to CQP without B-frames.

The arithmetic lives in the HIP library; this file only orders launches and owns device buffers.
"""
import ctypes as C
import math

import numpy as np

from .abi import STATE_FIELDS, CabacParams, CavlcParams, ChainCavlc, DeblockParams, MbState, NrState, SliceB, SliceParams, SliceRd
from . import quality
from .frame import LAMBDA_TAB, CqmDevice, DeviceArray, FrameCtx

SLICE_P, SLICE_B, SLICE_I = 0, 1, 2
I_4x4, I_8x8, I_16x16, I_PCM, P_L0, P_8x8, P_SKIP = range(7)
COST_SPAN = 2 * 4 * 2048      # p_cost_mv reaches +-2*4*2048 quarter-pels (R/encoder/analyse.c:191-198)

PAYLOAD_LEAD = 64
MB_BYTES_MAX = 8192          # SW_MB_BYTES_MAX (csrc/slice_kernel.h): the sweep stops before a macroblock whose worst case might not fit
MB_BYTES_AVG = 800           # what the default payload buffer provides per macroblock
LL_MB_BYTES = 6144           # ... for a lossless chain below the RD levels: no I_PCM candidate caps a macroblock there (derived beside SW_MB_BYTES_MAX)


def bframe_qp(qp, pb_factor=1.3):
    """rc->qp_constant[SLICE_TYPE_B] (R/encoder/ratecontrol.c:369-372)."""
    return min(max(int(qp + 6.0 * math.log(float(np.float32(pb_factor))) / math.log(2.0) + 0.5), 0), 51)


def coding_order(n_frames, keyint, bframes):
    """[(display index, slice type)] in coding order for a fixed pattern of `bframes` disposable B frames (x264_slicetype_decide
    without b-adapt, then x264_encoder_encode's reordering): an anchor every bframes + 1 frames after an IDR, the last frame before
    the next IDR / the end of the clip is an anchor too, every anchor is coded before the B frames it closes."""
    out, t = [], 0
    while t < n_frames:
        if (t % keyint == 0) if keyint > 0 else t == 0:
            out.append((t, SLICE_I))
            t += 1
            continue
        lim = min((t // keyint + 1) * keyint if keyint > 0 else n_frames, n_frames)
        anchor = min(t + bframes, lim - 1)
        out.append((anchor, SLICE_P))
        out += [(b, SLICE_B) for b in range(t, anchor)]
        t = anchor + 1
    return out


def iframe_qp(qp, ip_factor=1.4):
    """rc->qp_constant[SLICE_TYPE_I] (R/encoder/ratecontrol.c:370-372): the float ip_factor's log, truncated."""
    return min(max(int(qp - 6.0 * math.log(float(np.float32(ip_factor))) / math.log(2.0) + 0.5), 0), 51)


def rd_side_options(cabac, subme, trellis, psy_rd, psy_trellis, chroma_qp_offset):
    """x264_validate_parameters (R/encoder/encoder.c:493-522): what the RD-side options do to each other.  Returns (i_trellis, h->mb.i_psy_rd,
    h->mb.i_psy_trellis, i_chroma_qp_offset).  Host arithmetic only."""
    trellis = min(max(trellis, 0), 2) if cabac else 0
    psy_rd = 0.0 if subme < 6 else min(max(float(psy_rd), 0.0), 10.0)
    psy_rd_fix = int(np.float32(psy_rd) * 256 + 0.5)                  # FIX8
    # psy-trellis (--psy-rd A:B's B, :502-505,515): off without trellis, FIX8 of a quarter of the strength -- in the reference's float
    psy_trellis = min(max(float(psy_trellis), 0.0), 10.0) if trellis else 0.0
    psy_trellis_fix = psy_trellis_fix8(psy_trellis)
    # each lowers the chroma QP offset (:509-518); one clip after both (:521)
    if psy_rd_fix:
        chroma_qp_offset -= 1 if psy_rd < 0.25 else 2
    if psy_trellis_fix:
        chroma_qp_offset -= 1 if np.float32(psy_trellis) < 0.25 else 2
    return trellis, psy_rd_fix, psy_trellis_fix, min(max(chroma_qp_offset, -12), 12)


def psy_trellis_fix8(psy_trellis):
    """h->mb.i_psy_trellis of a VALIDATED strength (0 without trellis already): FIX8 of a quarter of it, in the reference's float."""
    return int(float(np.float32(psy_trellis) / np.float32(4) * np.float32(256)) + 0.5)


class DeviceState:
    """One x264hip_mb_state: allocated by the library, read back as numpy arrays [batch][n][...]."""

    def __init__(self, ctx, levels=True):
        self.ctx, self.st = ctx, MbState()
        # levels=False: X264HIP_STATE_NO_LEVELS -- no coefficient-level arrays (2/3 of a state's bytes), for sweeps that write the payload themselves
        ctx.check(ctx.lib.x264hip_mb_state_alloc_ex(ctx.h, C.byref(self.st), 0 if levels else 1), "mb_state_alloc")

    def get(self, name):
        d, B = self.ctx.dims, self.ctx.batch
        n = d.mb_w * d.mb_h
        _, dt, tail = next(f for f in STATE_FIELDS if f[0] == name)
        shape = (B, 8, n, 2) if name == "mvr" else (B, n) + tail
        out = np.zeros(shape, dt)
        rc = self.ctx.lib.x264hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), getattr(self.st, name), out.nbytes)
        assert rc == 0
        return out

    def free(self):
        self.ctx.lib.x264hip_mb_state_free(self.ctx.h, C.byref(self.st))


class ChainEncoder:
    """Encodes `batch` independent chains in lock step, frame t of every chain per sweep launch."""

    def __init__(self, lib, width, height, cqm, batch=1, qp=26, me_method=0, me_range=16, subme=0, n_refs=1, inter=0, intra=0,
                 transform8x8=0, fast_pskip=1, dct_decimate=1, chroma_me=1, cabac=0, deblock=0, alpha_c0=0, beta=0,
                 chroma_qp_offset=0, keyint=0, mixed_refs=0, noise_reduction=0, mv_range=0,
                 trellis=0, psy_rd=0.0, aq_mode=0, aq_strength=1.0, write=0, cabac_init_idc=0, qp_min=0, qp_max=51, payload_cap=0, raster=None,
                 bframes=0, weightb=0, direct_pred=1, lanes=0, levels=True, psnr=0, ssim=0, mb_stats=0, psy_trellis=0.0, cabac_pass=None, mb_carry=False,
                 cavlc_mp=None):
        self.lib = lib
        self.lossless = int(qp == 0)
        # param.analyse.b_psnr / b_ssim: the quality pass (quality.py) behind every frame -- a B frame's behind its sweep, on its unfiltered
        # reconstruction, a kept frame's behind the loop filter (x264_fdec_filter_row measures what it has just filtered, and b_deblock &= b_hpel).
        # mb_stats: the pass for h->stat.frame's counters alone (x264 counts macroblock types whether or not it measures).  Off by default: quality is
        # None and nothing is enqueued.  Lossless turns the two measurements off (R/encoder/encoder.c:410-411)
        self.quality = quality.flags(psnr and not self.lossless, ssim and not self.lossless, n_refs) if psnr or ssim or mb_stats else None
        self.reporters, self.last_report = {}, None
        if self.lossless:              # x264_validate_parameters, R/encoder/encoder.c:401-429: what constant QP 0 turns off (CQP: no adaptive quantisation)
            fast_pskip, noise_reduction, chroma_qp_offset, trellis, psy_rd, aq_mode = 0, 0, 0, 0, 0.0, 0
            transform8x8 = int(bool(transform8x8 and cabac))
            if not transform8x8:
                inter, intra = inter & ~2, intra & ~2
        trellis, self.psy_rd_fix, self.psy_trellis_fix, chroma_qp_offset = rd_side_options(cabac, subme, trellis, psy_rd, psy_trellis, chroma_qp_offset)
        aq_strength = min(max(float(aq_strength), 0.0), 3.0)
        aq_mode = 0 if aq_strength == 0 else min(max(aq_mode, 0), 1)
        # the raster-order variant of the sweep: needed by the RD levels, trellis, adaptive quantisation, or simply to get the payload
        # a CAVLC slice's payload is written by a pass over the state the sweep leaves (x264hip_cavlc_write_frame): CAVLC has no adaptive
        # state, so it needs no place in the macroblock loop and the wavefront variant stays the one that codes such slices (with adaptive
        # quantisation, and with B frames, which only the raster variant codes: the raster variant without its writer, whose QP rules leave
        # every macroblock's final QP in the state)
        self.cavlc = bool(write and not cabac and subme < 6 and not trellis)
        # cabac_pass: a CABAC slice below the RD levels is written the same way (x264hip_cabac_write_frame): the analysis there never reads the
        # contexts, so the wavefront variant codes it at constant QP and the raster variant without its writer under adaptive quantisation.
        # None keeps the in-loop writer and the selection as it was; True asks for the pass and refuses what it does not go with
        self.cabac_pass = bool(cabac_pass)
        if self.cabac_pass:
            why = ("cabac=0" if not cabac else "write=0" if not write else "subme >= 6 (the RD levels price against the live contexts)" if subme >= 6 else
                   "trellis" if trellis else "bframes (B slices keep the in-loop writer)" if bframes else "lossless" if self.lossless else
                   "levels=False (the pass reads the coefficient levels)" if not levels else "lanes" if lanes else None)
            if why:
                raise ValueError("cabac_pass=True does not go with %s" % why)
        # cavlc_mp: who writes a CAVLC slice wherever the CAVLC pass runs -- True: the macroblock-parallel pass (x264hip_cavlc_write_frame_mp /
        # _chains_mp: count, scan, place; every lane writes), None / False: the serial one (one lane per slice).  The bytes are the same
        self.cavlc_mp = bool(cavlc_mp)
        self._cavlc_mp_scratch = {}                    # per context (the main one, a lane's): the pass's scratch, live while its stream runs
        if self.cavlc_mp and not self.cavlc:
            raise ValueError("cavlc_mp=True does not go with %s: it selects the writer of the CAVLC pass (cabac=0, write=1, below the RD levels)" % (
                "cabac=1" if cabac else "write=0" if not write else "subme >= 6 or trellis (CAVLC under the RD levels is not built)"))
        in_loop = bool(write and not self.cavlc and not self.cabac_pass)
        self.raster = bool(subme >= 6 or trellis or aq_mode or in_loop or (self.cavlc and bframes)) if raster is None else bool(raster)
        self.rd_opt = dict(trellis=trellis, aq_mode=aq_mode, aq_strength=aq_strength, write=int(bool(in_loop or subme >= 6 or trellis)),
                           cabac_init_idc=cabac_init_idc, qp_min=qp_min, qp_max=qp_max)
        self.ctx = FrameCtx(lib, width, height, batch=batch)
        self.opt = dict(qp=qp, me_method=me_method, me_range=me_range, subme=subme, n_refs=n_refs, inter=inter, intra=intra,
                        transform8x8=transform8x8, fast_pskip=fast_pskip, dct_decimate=dct_decimate, chroma_me=chroma_me, cabac=cabac,
                        deblock=deblock, alpha_c0=alpha_c0, beta=beta, chroma_qp_offset=chroma_qp_offset, keyint=keyint, mixed_refs=mixed_refs,
                        noise_reduction=noise_reduction, mv_range=mv_range)
        self.cqm = CqmDevice(lib, cqm)
        self.cost = {}
        self.rd_bufs = None
        if self.raster:
            d, B = self.ctx.dims, batch
            n = d.mb_w * d.mb_h
            cap = payload_cap or (n * (LL_MB_BYTES if self.lossless and subme < 6 else MB_BYTES_AVG) + MB_BYTES_MAX + 128 + PAYLOAD_LEAD)
            rb = self._frame_bufs(B, n, cap, aq_mode)
            # p_cost_mv of every QP and the unquant tables, built by the library's host C (x264hip_cost_mv_table / _unquant_table)
            tabs = np.zeros((52, 2 * COST_SPAN + 1), np.int16)
            for q in range(52):
                lib.x264hip_cost_mv_table(LAMBDA_TAB[q], COST_SPAN, tabs[q].ctypes.data_as(C.c_void_p))
            rb["cost_mv_all"] = DeviceArray(lib, tabs.shape, np.int16, tabs)
            if "unquant4_mf" in cqm:                   # tables from frame.cqm_init (x264hip_cqm_init): complete
                u4, u8 = np.ascontiguousarray(cqm["unquant4_mf"], np.int32), np.ascontiguousarray(cqm["unquant8_mf"], np.int32)
            else:                                      # a table set without them (the reference's x264_cqm_init output as the tests hold it)
                q4 = np.ascontiguousarray(cqm["quant4_mf"][:, 6:12, :].astype(np.int32))       # the shift is zero at qp 6..11 (4x4) / 0..5 (8x8)
                q8 = np.ascontiguousarray(cqm["quant8_mf"][:, 0:6, :].astype(np.int32))
                u4, u8 = np.zeros((4, 52, 16), np.int32), np.zeros((2, 52, 64), np.int32)
                lib.x264hip_unquant_table(q4.ctypes.data_as(C.c_void_p), 4, 16, u4.ctypes.data_as(C.c_void_p))
                lib.x264hip_unquant_table(q8.ctypes.data_as(C.c_void_p), 2, 64, u8.ctypes.data_as(C.c_void_p))
            rb["unquant4_mf"] = DeviceArray(lib, u4.shape, np.int32, u4)
            rb["unquant8_mf"] = DeviceArray(lib, u8.shape, np.int32, u8)
            # x264hip_slice_rd.stale: the motion-cache entry that survives macroblocks and frames (read when temporal direct prediction
            # fails); one record per chain, zero like the reference's freshly allocated x264_t.  Per chain, and a chain's frames stay in
            # order, so temporal direct prediction also goes with the encoder that lets the chains drift apart (AsyncStreamEncoder)
            rb["stale"] = DeviceArray(lib, (B, 8), np.int16)
            # x264hip_slice_rd.psy_carry: h->mb.pic.fenc_dct4 | fenc_dct8, which the reference never clears either; zero like its x264_t
            if self.psy_trellis_fix:
                rb["psy_carry"] = DeviceArray(lib, (B, 512), np.int16)
            # x264hip_slice_rd.mb_carry: the macroblock's own non_zero_count / mvd cache entries, which the reference never resets either; with
            # sub-8x8 partitions under the RD levels the first partial trial encode of a macroblock prices against them.  Zero like its x264_t,
            # one record per chain, handed to every sweep and never reset.  Off by default: that combination then stays refused by the sweep
            if mb_carry:
                if bframes and inter & 0x20 and subme >= 6:
                    raise ValueError("mb_carry (sub-8x8 partitions with the RD levels) does not go with bframes: the B kernels do not keep the cache "
                                     "entries a macroblock leaves behind, and the sweep refuses a B slice of such a chain")
                rb["mb_carry"] = DeviceArray(lib, (B, 160), np.uint8, np.zeros((B, 160), np.uint8))
            self.rd_bufs = rb
            self.payload_cap = cap
        if self.cavlc and not levels:
            raise ValueError("CAVLC payloads are written from the coefficient levels: levels=False does not go with cabac=0, write=1")
        if (self.cavlc or self.cabac_pass) and not self.raster:
            d = self.ctx.dims
            n = d.mb_w * d.mb_h
            self.payload_cap = payload_cap or (n * MB_BYTES_AVG + MB_BYTES_MAX + 128 + PAYLOAD_LEAD)
            self.rd_bufs = self._frame_bufs(batch, n, self.payload_cap, 0)
        self.i_frame, self.i_frame_stride = 0, 0      # shard.py sets both when the chains are the GOPs of one stream
        self.import_ev = None          # upload_device with lanes: the event the lanes' streams wait for
        self._fenc = None              # the picture upload() fills: allocated on first use (a caller with its own source pictures never needs it)
        # B frames (disposable, one list-1 picture): encode_frame(src, stype, disp) in coding_order(); the DPB then holds
        # max(n_refs, 2) pictures (sps->vui.i_max_dec_frame_buffering, R/encoder/set.c:196-200)
        if bframes and direct_pred not in (1, 2) and not (direct_pred == 3 and getattr(self, "_direct_auto_ok", False)):
            # --direct auto picks a B frame's direct mode from running skip scores and evaluates BOTH modes in every macroblock (R/encoder/analyse.c:2476-2496,
            # encoder.c:113-118,1777-1790): the running scores are the stream encoder's (stream.py: x264hip_slice_b.direct_score); --direct none is not built
            raise ValueError("direct_pred %d: spatial (1) and temporal (2) direct prediction are built, --direct auto (3) in StreamEncoder (it needs the running "
                             "skip scores of the stream's B frames); --direct none is refused" % direct_pred)
        self.bopt = dict(bframes=bframes, weightb=int(bool(weightb)), direct_spatial=int(direct_pred != 2))
        self.dpb = max(n_refs, 2 if bframes else 1)
        self.pool = [self.ctx.new_picture() for _ in range(self.dpb + 1)]
        if not levels and not self.rd_opt["write"]:
            raise ValueError("levels=False: the coefficient levels are the only product unless the sweep writes the payload (write=1)")
        self.states = [DeviceState(self.ctx, levels) for _ in range(self.dpb + 1)]
        self.refs = []                 # [(picture, state, poc)], newest first (StreamEncoder.crefs: the same fields per chain)
        # lanes: the B frames between two anchors predict from the anchors only, never from each other, so they are independent
        # of one another and of the NEXT anchor.  With lanes = K each B frame is enqueued on one of K extra streams (own
        # reconstruction, state and payload buffers), ordered behind the anchor it needs by an event, and runs beside the
        # following anchor: a launch's slow chains no longer hold the whole device.  Same results, bit for bit.
        self.lanes, self.lane_i, self.anchor_ev, self.b_readers = [], 0, None, []
        if lanes and bframes:
            if not self.raster:
                raise ValueError("lanes: B frames run in the raster variant")
            if direct_pred == 2:
                raise ValueError("lanes: temporal direct prediction chains every frame to the one coded before it (x264hip_slice_rd.stale)")
            if noise_reduction:
                raise ValueError("lanes: --nr chains every frame to the one coded before it (x264hip_nr_state: its sums and the update behind every frame)")
            if self.psy_trellis_fix:
                raise ValueError("lanes: psy-trellis chains every frame to the one coded before it (x264hip_slice_rd.psy_carry)")
            d = self.ctx.dims
            for _ in range(lanes):
                lc = FrameCtx(lib, width, height, batch=batch)
                self.lanes.append(dict(ctx=lc, recon=lc.new_picture(source_only=True), state=DeviceState(lc, levels),
                                       bufs=self._frame_bufs(batch, d.mb_w * d.mb_h, self.payload_cap, aq_mode)))
        self.t = 0
        self.last_idr = 0
        self.profile = None            # DeviceArray [batch][mb_h][8] int64 when phase timing is wanted
        self.events = None             # set to [] to collect (start, stop, slice_type, n_refs) HIP events per sweep launch
        self.nr = None
        if noise_reduction:
            self.nr = NrState()
            self.ctx.check(lib.x264hip_nr_state_alloc(self.ctx.h, C.byref(self.nr)), "nr_state_alloc")

    def _frame_bufs(self, B, n, cap, aq_mode):
        """What one frame in flight writes: the payload, its length, the bit position after every macroblock, the AQ arrays."""
        lib = self.lib
        rb = dict(payload=DeviceArray(lib, (B, cap), np.uint8), payload_len=DeviceArray(lib, (B,), np.int32), mb_bits=DeviceArray(lib, (B, n), np.int32))
        if aq_mode:
            rb["aq_energy"] = DeviceArray(lib, (B, n), np.int32)
            rb["aq_offset"] = DeviceArray(lib, (B, n), np.float32)
        return rb

    def sync(self):
        """Everything enqueued so far, on the main stream and on the lanes, has finished."""
        self.ctx.sync()
        for ln in self.lanes:
            ln["ctx"].sync()

    def cost_table(self, qp):
        if qp not in self.cost:                        # p_cost_mv of this QP from the library's host C (x264hip_cost_mv_table), as cost_mv_all
            tab = np.zeros(2 * COST_SPAN + 1, np.int16)
            self.lib.x264hip_cost_mv_table(LAMBDA_TAB[qp], COST_SPAN, tab.ctypes.data_as(C.c_void_p))
            self.cost[qp] = DeviceArray(self.lib, tab.shape, np.int16, tab)
        return self.cost[qp]

    @property
    def fenc(self):
        if self._fenc is None:
            self._fenc = self.ctx.new_picture(source_only=True)
        return self._fenc

    def upload(self, y, u, v, b=0):
        for ln in self.lanes:          # a B frame still in flight on a lane may be reading this picture
            ln["ctx"].sync()
        self.ctx.upload(self.fenc, y, u, v, b=b)

    def upload_device(self, surfaces):
        """The same from pictures that already lie in device memory, any subset of the batch in one launch and without a synchronisation:
        surfaces as FrameCtx.import_surfaces takes them, [(element, csp, (ptr_y, ptr_u, ptr_v), (pitch_y, pitch_u, pitch_v))].  Unlike
        upload this returns before the picture is in place: what follows on the main stream is ordered behind it by the stream, and the
        lanes' streams are made to wait for it here."""
        L = self.lib
        for ln in self.lanes:          # a B frame still in flight on a lane may be reading this picture
            ln["ctx"].sync()
        self.ctx.import_surfaces(self.fenc, surfaces)
        if self.lanes:                 # a B frame coded next runs on a lane's own stream: behind the import, not beside it
            if self.import_ev is None:
                self.import_ev = L.x264hip_event_create()
                if not self.import_ev:
                    raise MemoryError("x264hip_event_create failed")
            self.ctx.check(L.x264hip_event_record(self.import_ev, self.ctx.stream), "event_record")
            for ln in self.lanes:
                self.ctx.check(L.x264hip_stream_wait_event(ln["ctx"].stream, self.import_ev), "stream_wait_event")

    # ---- the records a sweep is given: built here for every encoder of this package --------------------------------------------------
    def ref_lists(self, refs, poc, stype):
        """x264_reference_build_list (R/encoder/encoder.c:911-981) over [(picture, state, poc, ...)]: list 0 = earlier pictures, nearest
        first; list 1 = later ones."""
        l0 = sorted([r for r in refs if r[2] < poc], key=lambda r: -r[2])[:self.opt["n_refs"]] if stype != SLICE_I else []
        l1 = sorted([r for r in refs if r[2] > poc], key=lambda r: r[2])[:1] if stype == SLICE_B else []
        return l0, l1

    def slice_params(self, stype, qp, poc, cost_mv, lowres_mv):
        """x264hip_slice_params.  cost_mv: device address of p_cost_mv for this QP; lowres_mv: device address of the lookahead's vectors
        ([batch][n_mb][2] int16) or None.  ref_poc, rd and b are the caller's to fill."""
        o, b = self.opt, self.cqm.bufs
        return SliceParams(slice_type=stype, qp=qp, chroma_qp_offset=o["chroma_qp_offset"], me_method=o["me_method"], me_range=o["me_range"],
                           subme=o["subme"], chroma_me=o["chroma_me"], mv_range=o["mv_range"] or 512, fast_pskip=o["fast_pskip"], dct_decimate=o["dct_decimate"],
                           cabac=o["cabac"], transform8x8=o["transform8x8"], analyse_inter=o["inter"], analyse_intra=o["intra"],
                           quant4_mf=b["quant4_mf"].ptr, quant4_bias=b["quant4_bias"].ptr, quant8_mf=b["quant8_mf"].ptr,
                           quant8_bias=b["quant8_bias"].ptr, dequant4_mf=b["dequant4_mf"].ptr, dequant8_mf=b["dequant8_mf"].ptr,
                           cost_mv=cost_mv, cost_mv_range=COST_SPAN, poc=poc, mixed_refs=o["mixed_refs"],
                           profile=self.profile.ptr if self.profile else None,
                           noise_reduction=o["noise_reduction"], nr=C.addressof(self.nr) if self.nr else None, lossless=self.lossless,
                           lowres_mv=lowres_mv)

    def slice_rd(self, rb, f_qpm, i_frame, aq_offset, write, i_frame_stride):
        """x264hip_slice_rd for a frame that writes into the buffer set rb (_frame_bufs + the tables of rd_bufs).  aq_offset: device address
        of the frame's AQ offsets or None."""
        ro = self.rd_opt
        return SliceRd(trellis=ro["trellis"], psy_rd=self.psy_rd_fix, write=write, cabac_init_idc=ro["cabac_init_idc"], i_frame=i_frame,
                       qp_min=ro["qp_min"], qp_max=ro["qp_max"], f_qpm=f_qpm, aq_offset=aq_offset,
                       cost_mv_all=rb["cost_mv_all"].ptr, unquant4_mf=rb["unquant4_mf"].ptr, unquant8_mf=rb["unquant8_mf"].ptr,
                       payload=rb["payload"].ptr, payload_cap=self.payload_cap, payload_len=rb["payload_len"].ptr, mb_bits=rb["mb_bits"].ptr,
                       stale=rb["stale"].ptr, i_frame_stride=i_frame_stride, psy_trellis=self.psy_trellis_fix,
                       psy_carry=rb["psy_carry"].ptr if "psy_carry" in rb else None,
                       mb_carry=rb["mb_carry"].ptr if "mb_carry" in rb else None)

    def filter_kept(self, c, recon, s):
        """x264_fdec_filter_row for a whole kept frame, enqueued on context c: loop filter (from the x264hip_mb_state s), borders, half-pel
        planes."""
        L, o = self.lib, self.opt
        if o["deblock"]:
            dp = DeblockParams(mb_type=s.mb_type, qp=s.qp, nnz=s.nnz, transform8x8=s.t8, mv=s.mv, ref=s.ref,
                               alpha_c0_offset=o["alpha_c0"], beta_offset=o["beta"], chroma_qp_offset=o["chroma_qp_offset"], state_layout=1,
                               sub8x8=1 if o["inter"] & 0x20 else 0)
            c.check(L.x264hip_deblock_frame(c.h, C.byref(recon), C.byref(dp)), "deblock_frame")
        c.check(L.x264hip_expand_border(c.h, C.byref(recon), 0), "expand_border")
        c.check(L.x264hip_hpel_filter_frame(c.h, C.byref(recon)), "hpel_filter_frame")

    def encode_frame(self, src=None, stype=None, disp=None, lowres_mv=None, lowres_mv1=None):
        """The macroblock sweep for the frame held by `src` (default: the picture upload() fills) in every
        batch element.  Returns (slice_type, qp, state) -- the state's arrays are valid after ctx.sync().
        Without stype: I / P chains in display order (an IDR every keyint frames).  With stype / disp (see coding_order): the
        frame's slice type and display index, frames arriving in coding order -- the way B frames are coded."""
        L, c, o = self.lib, self.ctx, self.opt
        fenc = self.fenc if src is None else src
        if stype is None:
            idr = (self.t % o["keyint"] == 0) if o["keyint"] > 0 else self.t == 0
            stype, disp = (SLICE_I if idr else SLICE_P), self.t
        idr, is_b = stype == SLICE_I, stype == SLICE_B
        if idr:
            self.refs, self.last_idr = [], disp
        poc = 2 * (disp - self.last_idr)
        used = [r[0] for r in self.refs]
        lane = None
        if is_b and self.lanes:        # a lane's stream: behind the last anchor's filters, beside whatever else is in flight
            lane = self.lanes[self.lane_i % len(self.lanes)]
            self.lane_i += 1
            c, recon, state = lane["ctx"], lane["recon"], lane["state"]
            if self.anchor_ev:
                L.x264hip_stream_wait_event(c.stream, self.anchor_ev)
        else:
            pic_i = next(i for i, p in enumerate(self.pool) if not any(p is q for q in used))
            recon, state = self.pool[pic_i], self.states[pic_i]
            keep = []
            for ev, reads in self.b_readers:       # B frames on the lanes that still read the picture / state about to be overwritten
                if pic_i in reads:
                    L.x264hip_stream_wait_event(c.stream, ev)
                    reads.discard(pic_i)
                if reads:
                    keep.append((ev, reads))
                else:
                    L.x264hip_event_destroy(ev)
            self.b_readers = keep
        refs, refs1 = self.ref_lists(self.refs, poc, stype)
        qp = iframe_qp(o["qp"]) if idr else bframe_qp(o["qp"]) if is_b else o["qp"]      # (lossless: ip_factor = 1, and QP 0 stays 0 under the default's clamp)
        self.last_is_b, self.last_poc = is_b, poc
        p = self.slice_params(stype, qp, poc, self.cost_table(qp).ptr, lowres_mv.ptr if lowres_mv is not None else None)
        if self.raster:
            rb, ro = dict(self.rd_bufs, **lane["bufs"]) if lane else self.rd_bufs, self.rd_opt
            self.last_bufs = rb
            if ro["aq_mode"]:                  # x264_adaptive_quant_frame on the source (R/encoder/encoder.c:1421)
                c.check(L.x264hip_adaptive_quant_frame(c.h, C.byref(fenc), ro["aq_strength"], rb["aq_energy"].p, rb["aq_offset"].p), "adaptive_quant_frame")
            self.rd = self.slice_rd(rb, float(qp), self.i_frame, rb["aq_offset"].ptr if ro["aq_mode"] else None, ro["write"], self.i_frame_stride)
            p.rd = C.addressof(self.rd)
        if is_b:
            self.sb = SliceB(fref1=C.addressof(refs1[0][0]), l1_state=C.addressof(refs1[0][1].st), ref1_poc=refs1[0][2],
                             weightb=self.bopt["weightb"], direct_spatial=self.bopt["direct_spatial"],
                             lowres_mv1=lowres_mv1.ptr if lowres_mv1 is not None else None)
            p.b = C.addressof(self.sb)
        for i, r in enumerate(refs):
            p.ref_poc[i] = r[2]
        arr = (C.c_void_p * max(len(refs), 1))(*[C.addressof(r[0]) for r in refs]) if refs else None
        l0 = C.byref(refs[0][1].st) if refs else None
        ev = None
        if self.events is not None:            # HIP events on the launch stream around the sweep kernel (bench.py)
            ev = (L.x264hip_event_create(), L.x264hip_event_create())
            L.x264hip_event_record(ev[0], c.stream)
        c.check(L.x264hip_slice_sweep_frame(c.h, C.byref(fenc), arr, len(refs), C.byref(recon), C.byref(p), l0, C.byref(state.st)),
                "slice_sweep_frame")
        if ev:
            L.x264hip_event_record(ev[1], c.stream)
            self.events.append((ev[0], ev[1], stype, len(refs) + len(refs1)))
        if self.cavlc:                                 # x264_macroblock_write_cavlc for every macroblock of every chain, from the state just written
            rb = self.last_bufs if self.raster else self.rd_bufs       # (a B frame on a lane: the lane's payload buffers)
            cp = CavlcParams(slice_type=stype, n_ref0=len(refs), analyse_inter=o["inter"], transform8x8=o["transform8x8"], cqm_custom=0,
                             payload=rb["payload"].ptr, payload_cap=self.payload_cap, payload_len=rb["payload_len"].ptr, mb_bits=rb["mb_bits"].ptr,
                             slice_qp=qp)
            if self.cavlc_mp:
                c.check(L.x264hip_cavlc_write_frame_mp(c.h, C.byref(state.st), C.byref(cp), self.cavlc_mp_scratch(c).p), "cavlc_write_frame_mp")
            else:
                c.check(L.x264hip_cavlc_write_frame(c.h, C.byref(state.st), C.byref(cp)), "cavlc_write_frame")
            self.last_bufs = rb
        if self.cabac_pass:                            # x264_macroblock_write_cabac for every macroblock of every chain, from the state just written
            rb = self.last_bufs if self.raster else self.rd_bufs
            bp = CabacParams(slice_type=stype, n_ref0=len(refs), analyse_inter=o["inter"], transform8x8=o["transform8x8"], slice_qp=qp,
                             cabac_init_idc=self.rd_opt["cabac_init_idc"], i_frame=self.i_frame, i_frame_stride=self.i_frame_stride,
                             payload=rb["payload"].ptr, payload_cap=self.payload_cap, payload_len=rb["payload_len"].ptr, mb_bits=rb["mb_bits"].ptr)
            c.check(L.x264hip_cabac_write_frame(c.h, C.byref(state.st), C.byref(bp)), "cabac_write_frame")
            self.last_bufs = rb
        if self.nr:                            # x264_noise_reduction_update at the end of every frame (R/encoder/encoder.c:1755)
            c.check(L.x264hip_noise_reduction_update(c.h, C.byref(self.nr), o["noise_reduction"]), "noise_reduction_update")
        if lane:                               # whoever overwrites one of the pictures this frame reads waits for it
            ev = L.x264hip_event_create()
            L.x264hip_event_record(ev, c.stream)
            reads = {i for i, p in enumerate(self.pool) if any(p is r[0] for r in refs + refs1)}
            self.b_readers.append((ev, reads))
        self.last = (recon, state)
        self.last_ctx = c
        self.last_src, self.last_stype = fenc, stype
        if is_b and self.quality is not None:              # a disposable B frame is never filtered: measured as the sweep left it, on the stream it ran on
            self.measure(c, fenc, recon, state, stype)
        return stype, qp, state

    def cavlc_mp_scratch(self, c):
        """The device scratch of the macroblock-parallel CAVLC pass on context c, allocated on first use: x264hip_cavlc_mp_scratch_bytes for
        c.batch slices, the most one call writes (every chain's slice of a frame, or a chain table with at most one entry per chain)."""
        if id(c) not in self._cavlc_mp_scratch:
            self._cavlc_mp_scratch[id(c)] = DeviceArray(self.lib, (self.lib.x264hip_cavlc_mp_scratch_bytes(c.h, c.batch),), np.uint8)
        return self._cavlc_mp_scratch[id(c)]

    def measure(self, c, fenc, recon, state, stype):
        """The quality pass for the frame just coded, enqueued on context c (the main one or a lane's); reports() reads it after the sync."""
        if id(c) not in self.reporters:
            self.reporters[id(c)] = quality.Reporter(c, c.batch)
        self.last_report = self.reporters[id(c)].frame(fenc, recon, state.st, stype, self.quality)

    def reports(self):
        """x264hip_frame_report of the last frame of every chain (valid after sync(); a kept frame's after finish_frame): a numpy record
        array [batch] of quality.REPORT_DTYPE -- ssd, ssim (f_ssim, not yet divided), qp_sum and h->stat.frame's counters."""
        if self.last_report is None:
            raise RuntimeError("no quality pass was enqueued: ChainEncoder(psnr=1 / ssim=1), and finish_frame() for a kept frame")
        return quality.Reporter.records(self.last_report)

    def finish_frame(self):
        """x264_fdec_filter_row for the whole frame: loop filter, borders, half-pel planes; then the frame joins the reference list."""
        L, c, o = self.lib, self.ctx, self.opt
        recon, state = self.last
        if getattr(self, "last_is_b", False):          # a disposable B frame: neither filtered nor kept (R/encoder/encoder.c:986-1024,1060-1068)
            self.t += 1
            self.i_frame += 1
            return
        self.filter_kept(c, recon, state.st)
        if self.quality is not None:           # behind the loop filter, before the next upload overwrites the source
            self.measure(c, self.last_src, recon, state, self.last_stype)
        self.refs.insert(0, (recon, state, getattr(self, "last_poc", 2 * (self.t - self.last_idr))))
        del self.refs[self.dpb:]
        if self.lanes:                         # the point the B frames that predict from this anchor wait for
            if self.anchor_ev:
                L.x264hip_event_destroy(self.anchor_ev)
            self.anchor_ev = L.x264hip_event_create()
            L.x264hip_event_record(self.anchor_ev, c.stream)
        self.t += 1
        self.i_frame += 1

    def payloads(self):
        """slice_data() of the last frame of every chain (valid after ctx.sync()): list of bytes objects."""
        rb = getattr(self, "last_bufs", None) or self.rd_bufs
        n = rb["payload_len"].get()
        raw = rb["payload"].get()
        return [bytes(raw[b, PAYLOAD_LEAD:PAYLOAD_LEAD + n[b]]) for b in range(len(n))]

    def payload_async(self, b, host_len, host_buf, nbytes):
        """Enqueue, behind the sweep just launched, the copy of chain b's payload length and of the first `nbytes` bytes of its payload
        into pinned host memory (x264hip_host_alloc): no synchronisation, the bytes are there once the stream has passed this point."""
        rb = getattr(self, "last_bufs", None) or self.rd_bufs
        st = self.last_ctx.stream
        self.lib.x264hip_memcpy_d2h_async(host_len, rb["payload_len"].ptr + 4 * b, 4, st)
        self.lib.x264hip_memcpy_d2h_async(host_buf, rb["payload"].ptr + self.payload_cap * b + PAYLOAD_LEAD, nbytes, st)

    def status(self):
        c = self.ctx
        if getattr(self, "last", None) is None:          # nothing launched yet
            return
        c.check(self.lib.x264hip_slice_sweep_status(c.h, C.byref(self.last[1].st if not self.lanes or not self.last_is_b else self.states[0].st)), "slice_sweep_status")
        for ln in self.lanes:                  # each lane's context keeps its own sticky abort count
            ln["ctx"].check(self.lib.x264hip_slice_sweep_status(ln["ctx"].h, C.byref(ln["state"].st)), "slice_sweep_status")

    def close(self):
        for ev, _ in self.b_readers:
            self.lib.x264hip_event_destroy(ev)
        if self.anchor_ev:
            self.lib.x264hip_event_destroy(self.anchor_ev)
        if self.import_ev:
            self.lib.x264hip_event_destroy(self.import_ev)
        self.b_readers, self.anchor_ev, self.import_ev = [], None, None
        for r in self.reporters.values():
            r.close()
        self.reporters = {}
        if self.nr:
            self.lib.x264hip_nr_state_free(self.ctx.h, C.byref(self.nr))
            self.nr = None
        for ln in self.lanes:                  # each lane's payload / AQ buffers, state, reconstruction and stream
            for d in ln["bufs"].values():
                d.free()
            ln["state"].free()
            ln["ctx"].close()
        self.lanes = []
        for s in self.states:
            s.free()
        for d in list(self.cost.values()) + list(self._cavlc_mp_scratch.values()):
            d.free()
        self._cavlc_mp_scratch = {}
        for d in (self.rd_bufs or {}).values():
            d.free()
        self.cqm.free()
        self.ctx.close()
