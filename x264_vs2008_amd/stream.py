"""x264_encoder_encode for a batch of GOP chains with the real lookahead and rate control in front of the macroblock sweep
(R/encoder/encoder.c:1340-1600): x264_slicetype_decide places every chain's B frames (b-adapt 1 / 2, the pre-encode scene cut),
x264_ratecontrol_start prices every frame (CQP or CRF), and the lookahead's half-resolution vectors are the first candidates of the
16x16 searches -- so the chains stop moving in lock step: at one step chain A codes a P frame from references {9, 8} at QP 24 while
chain B codes a B frame between 8 and 12 at QP 27.

    enc = StreamEncoder(lib, w, h, cqm, batch=B, crf=23.0, bframes=3, b_adapt=1, ...)      # ChainEncoder's options + the lookahead's
    frames = enc.step(fill)                # one picture per chain in (fill(picture, input number)), at most one coded frame per chain out
    frames = enc.step(None)                # flushing: no more input; [] when every chain is done
    enc.payloads()                         # slice_data() of the frames just coded, per chain (None where the chain coded nothing)

Host side: x264_vs2008_amd.lookahead (the library's host C state machine per chain + the batched cost kernel).  Device side: one
chain-table launch per kernel kind (x264hip_slice_sweep_chains), each chain's entry naming its own source picture (the lookahead's slot),
references, reconstruction and QP; the end-of-frame filters run on the elements that coded a kept frame (x264hip_frame_ctx_elements).
The arithmetic lives in the HIP library; this file orders launches and owns device buffers."""
import ctypes as C
import os
import sys

import numpy as np

from . import lookahead as LA
from . import quality
from .abi import CavlcParams, ChainCavlc, ChainSweep, MbState, SliceB
from .frame import DeviceArray
from .slice import COST_SPAN, ChainEncoder, SLICE_B, SLICE_I, SLICE_P


class Coded:
    """What one chain coded in a step."""
    __slots__ = ("chain", "frame", "type", "slice_type", "qp", "f_qpm", "poc", "n_ref0", "n_ref1", "i_satd", "frame_num_reset", "direct_spatial", "report", "pic")

    def __repr__(self):
        return "Coded(chain=%d frame=%d type=%d qp=%d poc=%d)" % (self.chain, self.frame, self.type, self.qp, self.poc)


class StreamEncoder(ChainEncoder):
    def __init__(self, lib, width, height, cqm, batch=1, crf=None, b_adapt=1, bframe_bias=0, keyint_min=0, scenecut_threshold=40, pre_scenecut=1,
                 ip_factor=1.4, pb_factor=1.3, qcompress=0.6, qp_step=4, n_slots=0, speculative=True, limits=None, n_frames=None, lookahead_priority=False, b_cus=0, **kw):
        kw.setdefault("write", 1)
        if not kw.get("cabac", 0):
            # --no-cabac: the chain-table raster kernels without their writer leave decisions and levels in the states, one launch of
            # x264hip_cavlc_write_chains behind them writes every chain's slice.  Rate control and the post-encode scene cut read the states.
            if kw.get("subme", 0) >= 6:
                raise ValueError("StreamEncoder: cabac=0 with subme >= 6 (the RD levels price CAVLC bits with a counting twin of the writer: not built)")
            kw["trellis"] = 0                          # x264_validate_parameters: trellis needs CABAC
            kw.setdefault("levels", True)
            kw["raster"] = True
        kw.setdefault("levels", False)
        if kw.get("lanes"):
            raise ValueError("StreamEncoder: the chains of a step already run side by side; lanes belong to the lock-step encoder")
        self._direct_auto_ok = True                     # --direct auto: the running scores live here (c_dscore)
        # sub-8x8 partitions with the RD levels (--partitions all --subme 6..9): every chain's frames are swept in its coding order here, the
        # given-up attempts of the post-encode scene cut included, so the chain's record of cache leftovers (x264hip_slice_rd.mb_carry) is on
        if kw.get("inter", 0) & 0x20 and kw.get("subme", 0) >= 6 and kw.get("qp", 26) != 0:
            if kw.get("bframes", 0):
                raise ValueError("StreamEncoder: sub-8x8 partitions (inter & 0x20) with the RD levels (subme >= 6) and bframes > 0: the B kernels do not "
                                 "keep the cache entries a macroblock leaves behind (x264hip_slice_rd.mb_carry); I / P streams are built")
            kw["mb_carry"] = True
        super().__init__(lib, width, height, cqm, batch=batch, **kw)
        if not self.raster or not (self.rd_opt["write"] or self.cavlc):
            raise ValueError("StreamEncoder: the chain-table sweep is the raster variant with the entropy coder in the loop, or followed by the CAVLC pass")
        o, d = self.opt, self.ctx.dims
        if self.lossless:              # x264_validate_parameters (R/encoder/encoder.c:401-417): constant QP 0 for every frame type, no B frames
            crf, ip_factor, pb_factor = None, 1.0, 1.0
            if self.bopt["bframes"]:
                raise ValueError("StreamEncoder: lossless (qp 0) has no B frames (x264_validate_parameters sets bframes = 0)")
        keyint = o["keyint"] if o["keyint"] > 0 else 1 << 30
        self.la_params = LA.make_params(d.mb_w, d.mb_h, bframes=self.bopt["bframes"], b_adapt=b_adapt if self.bopt["bframes"] else 0, bframe_bias=bframe_bias,
                                        keyint_max=keyint, keyint_min=keyint_min, scenecut_threshold=scenecut_threshold, pre_scenecut=pre_scenecut,
                                        crf=crf, qp=o["qp"], ip_factor=ip_factor, pb_factor=pb_factor, qcompress=qcompress,
                                        qp_min=self.rd_opt["qp_min"], qp_max=self.rd_opt["qp_max"], qp_step=qp_step)
        bf = self.bopt["bframes"]
        delay = (max(bf, 3) * 4 if b_adapt == 2 and bf else bf)
        self.n_slots = n_slots or (delay + bf + 3)        # oldest live frame .. newest input spans at most delay + bframes + 2 (asserted when a slot is reused)
        # The lookahead works on a stream of its own (same geometry, so its pictures are the sweep's sources): with n_frames given (how many
        # pictures every chain will take) step() prepares the NEXT call's decisions right after launching this one's sweep, and the
        # lookahead's kernels fill the wave slots the step's B chains leave when they finish ahead of its P chains.
        from .frame import FrameCtx
        # b_cus: the step's B kernel on compute units [0, b_cus), its I / P kernel (and everything else of this context) on the rest
        self._cu_streams = []
        if b_cus:
            sb_, sp_ = lib.x264hip_stream_create_cu_range(0, b_cus), lib.x264hip_stream_create_cu_range(b_cus, 256 - b_cus)
            if not sb_ or not sp_:
                raise RuntimeError("x264hip_stream_create_cu_range failed")
            self._cu_streams = [sb_, sp_]
            old = self.ctx
            self.ctx = FrameCtx(lib, width, height, stream=sp_, batch=batch)         # same geometry: the pool's pictures and states stay where they are
            self.ctx.pictures, old.pictures = old.pictures, []
            for st_ in self.states:
                st_.ctx = self.ctx
            old.close()
            self.ctx.check(lib.x264hip_frame_ctx_set_b_stream(self.ctx.h, sb_), "frame_ctx_set_b_stream")
        self._hp_stream = None
        if lookahead_priority:
            self._hp_stream = lib.x264hip_stream_create_high_priority()
        self.src_ctx = FrameCtx(lib, width, height, stream=self._hp_stream, batch=batch)
        self.n_frames = n_frames
        self._prep = None
        self._coding = set()
        self.look = LA.LookaheadDevice(self.src_ctx, self.n_slots, bf, me_method=o["me_method"], me_range=o["me_range"], weightb=self.bopt["weightb"],
                                       bframe_bias=bframe_bias, subme=o["subme"], lossless=self.lossless)
        self.lb = LA.LookaheadBatch(self.src_ctx, self.la_params, self.look, speculative=speculative, limits=limits)
        B, n = batch, d.mb_w * d.mb_h
        # fenc->f_qp_offset of every slot (x264_adaptive_quant_frame runs when the picture comes in, encoder.c:1420-1421)
        self.aq_slots = None
        if self.rd_opt["aq_mode"]:
            self.aq_slots = [(DeviceArray(lib, (B, n), np.int32), DeviceArray(lib, (B, n), np.float32)) for _ in range(self.n_slots)]
        # per chain: [(picture, MbState copy with this chain's frame-level scalars, poc, pool index)], newest first (ChainEncoder.refs' fields
        # and the pool index); the IDR's input number; frames coded
        self.crefs = [[] for _ in range(B)]
        self.c_last_idr = [0] * B
        self.c_coded = [0] * B
        tb = lib.x264hip_chain_sweep_bytes()
        self.tab_host = lib.x264hip_host_alloc(tb * B)
        self.tab_dev = DeviceArray(lib, (tb * B,), np.uint8)
        self.elems_dev = [DeviceArray(lib, (B,), np.int32) for _ in range(len(self.pool))]
        # --nr: the chains that coded a frame for good in a step, for x264hip_noise_reduction_update_chains (_nr_update)
        self.nr_chains_dev = DeviceArray(lib, (B,), np.int32) if self.nr else None
        self.cv_host, self.cv_dev, self._cv = None, None, []       # the table of x264hip_cavlc_write_chains; what _entry notes for it
        if self.cavlc:
            cvb = lib.x264hip_chain_cavlc_bytes()
            self.cv_host = lib.x264hip_host_alloc(cvb * B)
            self.cv_dev = DeviceArray(lib, (cvb * B,), np.uint8)
        self.flushing = False
        self.coded_now = [None] * B
        self.n_sweeps = 0
        # --direct auto (h->mb.b_direct_auto_write): every B macroblock predicts both direct modes and credits each with the skip it would give
        # (the sweep leaves the frame's two sums in dscore_dev); h->stat.i_direct_score, the running scores that pick the next B frame's mode
        # (encoder.c:113-118) and decay as x264_encoder_frame_end lets them (:1777-1790), are kept per chain here
        self.direct_auto = bool(self.bopt["bframes"] and kw.get("direct_pred", 1) == 3)
        self.dscore_dev = DeviceArray(lib, (B, 2), np.int32) if self.direct_auto else None
        self.c_dscore = [[0, 0] for _ in range(B)]
        self._dscore_pending = []
        # Without --pre-scenecut the reference looks at every P frame AFTER coding it (x264_encoder_encode, encoder.c:1603-1699) and, if it finds a
        # scene cut, codes again: the picture as I / IDR, or the B picture before it as the P.  The decision is made from the sweep's own
        # statistics (x264hip_frame_stats + x264hip_scenecut_post), the queue surgery by the library (x264hip_lookahead_scenecut), the second
        # attempt inside the same step (step()).
        self.post_scenecut = bool(scenecut_threshold >= 0 and not pre_scenecut)
        self._post, self.stats_dev, self._undo, self.n_given_up = [], None, {}, 0
        if self.post_scenecut:
            if o["keyint"] <= 0:
                raise ValueError("StreamEncoder: the post-encode scene cut needs a finite keyint")
            self.stats_dev = [DeviceArray(lib, (B, 32), np.uint8) for _ in self.pool]
        self.sweep_events = None       # set to [] to collect (start, stop, chains, algorithmic bytes) HIP events around every step's sweep launches
        # psnr / ssim (ChainEncoder's options): ONE quality pass per launch over the chains that coded a frame, behind the kept frames' loop filter
        # (the B frames' reconstructions stay unfiltered), every entry naming its chain's source slot, pool picture and state (quality.Reporter.chains)
        self._q, self._reporter = [], None

    # ---- one call of x264_encoder_encode for every chain --------------------------------------------------------------------------
    def _prepare(self, fill):
        """The lookahead's part of one x264_encoder_encode call for every chain: a picture comes in (or the flush begins), the queues decide.
        Runs on the lookahead's stream; everything it launched has finished when it returns."""
        self._put(fill)
        return self._decide()

    def _put(self, fill):
        """The picture comes in (x264_encoder_encode up to the frame queue: copy, lowres planes, intra costs, adaptive quantisation)."""
        more = fill is not None and (self.n_frames is None or self.lb.fed < self.n_frames)
        if not more:
            self.flushing = True
        else:
            # the slot the new picture takes must not be one a sweep still in flight reads (possible only when the ring is at its bound)
            if self.look.frame_of_slot[self.look.slot(self.lb.fed)] in self._coding:
                self.ctx.sync()
            self.lb.put(lambda pic, f: self._fill(fill, pic, f))

    def _decide(self):
        """The queues decide (x264_slicetype_decide, x264_rc_analyse_slice, x264_ratecontrol_start) with the cost kernel behind them."""
        frames = self.lb.get(self.flushing)
        self.src_ctx.sync()
        return frames

    def step(self, fill):
        """fill(picture, frame): write input picture `frame` of every chain into `picture` (enc.src_ctx.upload / .synth / .import_surfaces); None: flush.
        Pictures that already lie in device memory (a decoder's NV12 surfaces) come in with one launch for all chains and no synchronisation;
        a chain that has run out of input is simply not named and keeps its element:

            def fill(picture, frame):
                enc.src_ctx.import_surfaces(picture, [(b, CSP_NV12, (s.y_ptr, s.uv_ptr, None), (s.pitch, s.pitch, 0))
                                                      for b, s in enumerate(decoded[frame]) if s is not None])

        Returns the list of Coded for the chains that coded a frame (empty while the B buffer fills; empty for good once flushed).
        With n_frames given to the constructor the next call's lookahead is prepared before this one returns (fill is then also asked
        for the following picture) and the flush starts by itself after n_frames pictures."""
        # with n_frames known the next call's lookahead (picture in, costs, decisions) runs beside this call's sweep
        frames = self._prep if self._prep is not None else self._prepare(fill)
        self._prep = None
        self.coded_now = [None] * self.ctx.batch
        pipelined = self.n_frames is not None
        if not any(fr is not None for fr in frames):
            self._coding = set()
            if pipelined and not self.flushing:
                self._prep = self._prepare(fill)
            return []
        out = self._sweep(frames)
        if not self.post_scenecut:
            self._nr_update(out)
            if pipelined and not self.flushing:
                self._prep = self._prepare(fill)        # beside the sweep just launched
            return out
        # x264_encoder_encode looks at the P picture it just coded (encoder.c:1603-1699) and, if an intra picture would have been as good, gives the
        # attempt up and codes again -- the same picture as I / IDR or the B picture before it as the P -- inside the same call.  Here: wait for the
        # sweep, ask (x264hip_frame_stats + x264hip_scenecut_post), and run the given-up chains again until none is left.  Each round costs a whole
        # frame time for a few chains: fine for a handful of streams, a reason to decide scene cuts in the lookahead (pre_scenecut = 1) for thousands.
        # The next call's lookahead does not wait for the verdicts: it runs ahead beside the sweep, on the assumption that nothing is given up,
        # with a copy of the judged chains' queues to come back to (x264hip_lookahead_save / _restore).
        done = [cd.chain for cd in out]
        judged = sorted({ci for _, ci, _, _ in self._post})
        saved = None
        if pipelined and not self.flushing:
            saved = {ci: self.lb.chains[ci].save() for ci in judged}
            if any(v is None for v in saved.values()):
                saved = None
        if saved is not None:
            self.lb.end(done)
            self._prep = self._prepare(fill)
        redone = []
        while True:
            self.ctx.sync()
            hits = self._scenecut_hits()
            if not hits:
                break
            for ci in hits:
                if saved is not None and ci not in redone:
                    self.lb.chains[ci].restore(saved[ci])
                self._give_up(ci)
            redone += [ci for ci in hits if ci not in redone]
            again = self.lb.get(self.flushing, only=hits)
            self.src_ctx.sync()
            redo = {cd.chain: cd for cd in self._sweep(again)}
            out = [redo.get(cd.chain, cd) for cd in out]
            self.n_given_up += len(hits)
        if saved is None:
            self.lb.end(done)
        elif redone:                                    # their decisions for the next call were made on the wrong assumption: made again
            self.lb.end(redone)
            nxt = self.lb.get(self.flushing, only=redone)
            self.src_ctx.sync()
            for ci in redone:
                self._prep[ci] = nxt[ci]
        self._nr_update(out)
        return out

    def _nr_update(self, out):
        """x264_noise_reduction_update for the chains that coded a frame for good in this step (encoder.c:1755: once per returned frame, behind
        the `goto do_encode` of a given-up attempt, whose additions to the sums stay): one call behind the step's last sweep, none between the
        attempts, and a chain that coded nothing keeps its tables as they are (the update halves: it is not idempotent)."""
        if not self.nr or not out:
            return
        c = self.ctx
        lst = np.zeros(c.batch, np.int32)
        lst[:len(out)] = [cd.chain for cd in out]
        self.nr_chains_dev.set(lst)
        c.check(self.lib.x264hip_noise_reduction_update_chains(c.h, C.byref(self.nr), self.opt["noise_reduction"], self.nr_chains_dev.p, len(out)),
                "noise_reduction_update_chains")

    def _sweep(self, frames):
        """The chain-table launch for the chains that have a frame in `frames` (per chain an x264hip_look_frame or None), then the filters of the kept ones."""
        L, c = self.lib, self.ctx
        todo = [(ci, fr) for ci, fr in enumerate(frames) if fr is not None]
        if self._dscore_pending:                        # the B frames of the last sweep: their skip sums join the running scores before the next mode is picked
            c.sync()
            fs, n_mb = self.dscore_dev.get(), c.dims.mb_w * c.dims.mb_h
            for ci in self._dscore_pending:
                sc = self.c_dscore[ci]
                if sc[0] + sc[1] > n_mb:
                    sc[0], sc[1] = sc[0] * 9 // 10, sc[1] * 9 // 10
                sc[0] += int(fs[ci][0]); sc[1] += int(fs[ci][1])
            self._dscore_pending = []
        # (c.sync: the previous step's sweep and filters are done: their tables, element lists and pictures are free)
        out, keep, filt, ev = self._launch(c, todo, self.tab_host, self.tab_dev.p, self._publish_elements, c.sync)
        if ev:
            px = self.ctx.dims.mb_w * 16 * self.ctx.dims.lines_y
            # per frame the source (1.5 B/px), each reference's four luma planes + chroma (4.5 B/px) and the reconstruction (1.5 B/px)
            self.sweep_events.append((ev[0], ev[1], len(todo), sum(px * (3.0 + 4.5 * (cd.n_ref0 + cd.n_ref1)) for cd in out),
                                      "".join("PBI"[cd.slice_type] for cd in out[:1]) + ":%d" % len(todo)))
        self.n_sweeps += 1
        if self.post_scenecut:
            self._post = []
            for pic_i, chains in filt.items():
                ps = [ci for ci in chains if self.coded_now[ci].slice_type == SLICE_P]
                if ps:
                    c.check(L.x264hip_frame_stats(c.h, C.byref(self.states[pic_i].st), self.stats_dev[pic_i].p), "frame_stats")
                    self._post += [(pic_i, ci, self.coded_now[ci].frame, self.coded_now[ci].frame - self.c_last_idr[ci]) for ci in ps]
        self._keep = keep
        if not self.post_scenecut:
            self.lb.end([ci for ci, _ in todo])
        self.last_bufs, self.last_ctx = self.rd_bufs, c
        self._coding = {cd.frame for cd in out}
        return out

    def _publish_elements(self, pic_i, chains):
        """The element list of pool picture pic_i for x264hip_frame_ctx_elements: uploaded to the picture's own device array."""
        el = self.elems_dev[pic_i]
        lst = np.zeros(self.ctx.batch, np.int32)
        lst[:len(chains)] = chains
        el.set(lst)
        return el.p

    def _launch(self, c, pairs, tab_host, tab_dev, publish, ready, done_events=None):
        """One chain-table launch on context c for the (chain, x264hip_look_frame) pairs, then x264_fdec_filter_row for the kept frames on the
        elements that were just written.  tab_host / tab_dev: the launch's table buffers; publish(pool picture, chains): the address of
        that picture's element list, the chains in it; ready(): called once the entries are built, before anything is enqueued -- whatever
        the launch reads or overwrites is free after it; done_events: (I / P kernel, B kernel) completion events, or None.
        Returns (out, keep, filt, ev): the Coded records, what the C calls read and must outlive them, {pool picture: chains that kept it},
        the two timing events around the launch if self.sweep_events collects them."""
        L = self.lib
        keep, written, filt, out = [], set(), {}, []
        self._cv, self._q = [], []
        entries = (ChainSweep * len(pairs))()
        for k, (ci, fr) in enumerate(pairs):
            entries[k], cd, pic_i = self._entry(ci, fr, keep)
            written.add(pic_i)
            out.append(cd)
            if cd.slice_type != SLICE_B:                   # kept: filtered below
                filt.setdefault(pic_i, []).append(ci)
        ready()
        for pic_i in written:
            c.check(L.x264hip_mb_state_clear_progress(c.h, C.byref(self.states[pic_i].st)), "mb_state_clear_progress")
        ev = None
        if self.sweep_events is not None:
            ev = (L.x264hip_event_create(), L.x264hip_event_create())
            L.x264hip_event_record(ev[0], c.stream)
        if done_events:
            c.check(L.x264hip_slice_sweep_chains_events(c.h, entries, len(pairs), tab_host, tab_dev, done_events[0],
                                                        done_events[1]), "slice_sweep_chains_events")
        else:
            c.check(L.x264hip_slice_sweep_chains(c.h, entries, len(pairs), tab_host, tab_dev), "slice_sweep_chains")
        if ev:
            L.x264hip_event_record(ev[1], c.stream)
        if self.cavlc:                                     # every chain's slice from the state its sweep just wrote: I, P and B chains in one launch
            cv = (ChainCavlc * len(self._cv))()
            for k, (ci, mine, cp) in enumerate(self._cv):
                cv[k] = ChainCavlc(ci, C.addressof(mine), C.addressof(cp))
            if self.cavlc_mp:                              # (scratch for a full table: a step holds at most one entry per chain)
                c.check(L.x264hip_cavlc_write_chains_mp(c.h, cv, len(self._cv), self.cv_host, self.cv_dev.p, self.cavlc_mp_scratch(c).p),
                        "cavlc_write_chains_mp")
            else:
                c.check(L.x264hip_cavlc_write_chains(c.h, cv, len(self._cv), self.cv_host, self.cv_dev.p), "cavlc_write_chains")
        for pic_i, chains in filt.items():
            c.check(L.x264hip_frame_ctx_elements(c.h, publish(pic_i, chains), len(chains)), "frame_ctx_elements")
            self.filter_kept(c, self.pool[pic_i], self.states[pic_i].st)
        c.check(L.x264hip_frame_ctx_elements(c.h, None, 0), "frame_ctx_elements")
        if self.quality is not None:                       # x264_fdec_filter_row's measurement and x264_slice_write's counters, all chains in one enqueue
            if done_events:
                raise ValueError("psnr / ssim: a launch whose B kernel ends on a stream of its own is not measured (StreamEncoder and ChainEncoder are)")
            if self._reporter is None:
                self._reporter = quality.Reporter(c, c.batch)
            ps, ss, rf = self.quality & quality.REPORT_PSNR, self.quality & quality.REPORT_SSIM, self.quality & quality.REPORT_REFS
            h = self._reporter.chains([(ci, self.look.pics[slot], ci, self.pool[pic_i], ci, mine, stype, ps, ss, rf) for ci, slot, pic_i, mine, stype in self._q])
            for k, cd in enumerate(out):
                cd.report = (h, k)
        return out, keep, filt, ev

    def report_of(self, cd):
        """The x264hip_frame_report (a quality.REPORT_DTYPE record) of a Coded this encoder returned; valid after sync(), until 8 further launches."""
        if cd.report is None:
            raise RuntimeError("no quality pass was enqueued: StreamEncoder(psnr=1 / ssim=1)")
        return quality.Reporter.records(cd.report[0])[cd.report[1]]

    def _scenecut_hits(self):
        """After sync(): the chains whose P picture of the last sweep the reference would give up (encoder.c:1603-1644)."""
        if not self._post:
            return []
        L, d, lp = self.lib, self.ctx.dims, self.la_params
        got, hits = {}, []
        for pic_i, ci, frame, gop in self._post:
            if pic_i not in got:
                got[pic_i] = self.stats_dev[pic_i].get()
            rec = np.ascontiguousarray(got[pic_i][ci])
            if L.x264hip_scenecut_post(rec.ctypes.data_as(C.c_void_p), d.mb_w * d.mb_h, gop, lp.scenecut_threshold, lp.keyint_min, lp.keyint_max):
                hits.append(ci)
        self._post = []
        return hits

    def _give_up(self, ci):
        """The attempt of chain ci is dropped: its reconstruction never joined the DPB, its payload is never read, its frame was never counted
        (x264_reference_update and x264_encoder_frame_end are not reached for it); the chain's queue rearranges itself (x264hip_lookahead_scenecut)."""
        self.crefs[ci], self.c_coded[ci] = self._undo[ci]
        self.coded_now[ci] = None
        self.lb.chains[ci].scenecut()
        self.lb.pending[ci] = None

    def _entry(self, ci, fr, keep):
        """One chain's sweep for the frame its queue handed it: the x264hip_chain_sweep record (whatever it points at goes into `keep`), the
        chain's DPB bookkeeping (x264_reference_build_list before, x264_reference_update after), the Coded record, the pool picture written."""
        rb = self._bufs_of(ci)
        idr = fr.type == LA.TYPE_IDR
        stype = SLICE_I if fr.type in (LA.TYPE_IDR, LA.TYPE_I) else SLICE_B if fr.type == LA.TYPE_B else SLICE_P
        if idr:
            self.crefs[ci], self.c_last_idr[ci] = [], fr.frame
        refs_all = self.crefs[ci]
        poc = fr.poc
        used = {r[3] for r in refs_all}
        pic_i = next(i for i in range(len(self.pool)) if i not in used)
        recon, state = self.pool[pic_i], self.states[pic_i]
        refs, refs1 = self.ref_lists(refs_all, poc, stype)
        qp = fr.qp
        slot = self.look.slot(fr.frame)
        assert self.look.frame_of_slot[slot] == fr.frame, "input frame %d left its lookahead slot before it was coded (n_slots too small)" % fr.frame
        lw0 = lw1 = None
        n = self.look.n
        if stype != SLICE_I and fr.lowres_l0:     # the kernel adds the chain's offset in an [batch][n_mb][2] array to the pointer it is given
            lw0 = self.look.mv_ptr(ci, fr.frame, 0, fr.frame - fr.ref0_frame) - 4 * n * ci
        if stype == SLICE_B and fr.lowres_l1:
            lw1 = self.look.mv_ptr(ci, fr.frame, 1, fr.ref1_frame - fr.frame) - 4 * n * ci
        # (cost_mv: a row of the table of all QPs: no allocation while kernels run -- hipMalloc waits for the device)
        p = self.slice_params(stype, qp, poc, rb["cost_mv_all"].ptr + qp * (2 * COST_SPAN + 1) * 2, lw0)
        rd = self.slice_rd(rb, fr.f_qpm, self.c_coded[ci], self.aq_slots[slot][1].ptr if self.aq_slots else None, 0 if self.cavlc else 1, 0)
        p.rd = C.addressof(rd)
        keep += [p, rd]
        dsp = self.bopt["direct_spatial"]
        if stype == SLICE_B:
            if self.direct_auto:                       # x264_slice_header_init, encoder.c:113-118
                dsp = int(self.c_dscore[ci][1] > self.c_dscore[ci][0])
                self._dscore_pending.append(ci)
            sb = SliceB(fref1=C.addressof(refs1[0][0]), l1_state=C.addressof(refs1[0][1]), ref1_poc=refs1[0][2],
                        weightb=self.bopt["weightb"], direct_spatial=dsp, lowres_mv1=lw1,
                        direct_score=self.dscore_dev.ptr if self.direct_auto else None)
            p.b = C.addressof(sb)
            keep.append(sb)
        for i, r in enumerate(refs):
            p.ref_poc[i] = r[2]
        arr = (C.c_void_p * max(len(refs), 1))(*[C.addressof(r[0]) for r in refs]) if refs else None
        mine = MbState.from_buffer_copy(state.st)        # this chain's view of the state: the device arrays + its own frame-level scalars
        keep += [arr, mine]
        if self.cavlc:
            cp = CavlcParams(slice_type=stype, n_ref0=len(refs), analyse_inter=self.opt["inter"], transform8x8=self.opt["transform8x8"], cqm_custom=0,
                             payload=rb["payload"].ptr, payload_cap=self.payload_cap, payload_len=rb["payload_len"].ptr, mb_bits=rb["mb_bits"].ptr,
                             slice_qp=qp)
            keep.append(cp)
            self._cv.append((ci, mine, cp))
        entry = ChainSweep(ci, C.addressof(self.look.pics[slot]), C.cast(arr, C.c_void_p) if arr else None, len(refs), C.addressof(recon),
                                C.addressof(p), C.addressof(refs[0][1]) if refs else None, C.addressof(mine))
        cd = Coded()
        cd.chain, cd.frame, cd.type, cd.slice_type, cd.qp, cd.f_qpm, cd.poc = ci, fr.frame, fr.type, stype, qp, fr.f_qpm, poc
        cd.n_ref0, cd.n_ref1, cd.i_satd = len(refs), len(refs1), fr.i_satd
        cd.frame_num_reset = int(getattr(fr, "frame_num_reset", 0))
        cd.direct_spatial = dsp
        cd.report = None
        cd.pic = pic_i                                 # the pool picture (and state) this frame was coded into
        self._q.append((ci, slot, pic_i, mine, stype))
        self._undo[ci] = (list(refs_all), self.c_coded[ci])
        self.coded_now[ci] = cd
        if stype != SLICE_B:                           # kept: filtered below, then this chain's newest reference
            self.crefs[ci] = ([(recon, mine, poc, pic_i)] + refs_all)[:self.dpb]
        self.c_coded[ci] += 1
        return entry, cd, pic_i

    def _bufs_of(self, ci):
        """The buffers the chain's next frame writes (AsyncStreamEncoder alternates two sets per chain)."""
        return self.rd_bufs

    def _fill(self, fill, pic, frame):
        fill(pic, frame)
        if self.aq_slots:
            c, L, ro = self.src_ctx, self.lib, self.rd_opt
            en, off = self.aq_slots[self.look.slot(frame)]
            c.check(L.x264hip_adaptive_quant_frame(c.h, C.byref(pic), ro["aq_strength"], en.p, off.p), "adaptive_quant_frame")

    def payloads(self):
        """slice_data() of the frame each chain coded in the last step (None where it coded nothing); valid after sync()."""
        all_ = super().payloads()
        return [p if self.coded_now[i] is not None else None for i, p in enumerate(all_)]

    def status(self):
        c = self.ctx
        for s in self.states:
            c.check(self.lib.x264hip_slice_sweep_status(c.h, C.byref(s.st)), "slice_sweep_status")

    def close(self):
        self.sync()
        self.src_ctx.sync()
        if self._reporter is not None:
            self._reporter.close()
            self._reporter = None
        self.lb.close()
        self.look.close()
        for pair in self.aq_slots or []:
            for a in pair:
                a.free()
        for a in [self.tab_dev] + self.elems_dev + ([self.nr_chains_dev] if self.nr_chains_dev else []) + (self.stats_dev or []) + ([self.dscore_dev] if self.dscore_dev else []) + ([self.cv_dev] if self.cv_dev else []):
            a.free()
        if self.cv_host:
            self.lib.x264hip_host_free(self.cv_host)
            self.cv_host = None
        if self.tab_host:
            self.lib.x264hip_host_free(self.tab_host)
            self.tab_host = None
        super().close()
        self.src_ctx.close()
        if self._hp_stream:
            self.lib.x264hip_stream_destroy(self._hp_stream)
            self._hp_stream = None


class AsyncStreamEncoder(StreamEncoder):
    """The same streams without the step: every chain gets its next frame as soon as ITS OWN kernel is done.

    In StreamEncoder a step ends when its slowest chain does; a P chain's frame takes about twice as long as a B chain's, so the wave slots
    of the B chains idle for the rest of every step.  Here a host scheduler polls the completion of the I / P kernel and of the B kernel of
    every launch in flight (x264hip_slice_sweep_chains_events, x264hip_event_query), asks the freed chains' queues for their next frames
    (batching the lookahead's cost requests over them) and launches those at once, on one of a small ring of contexts (streams) -- so
    launches of different "ages" overlap and the device stays full.  Chains therefore drift apart: a picture is prepared for ALL chains
    (lowres planes, intra costs, AQ) when the first chain needs it, and the slot ring is `drift` pictures longer; a chain that would run
    further ahead than the ring allows waits.  The results per chain are exactly StreamEncoder's (tests/test_gpu_stream.py).

        enc = AsyncStreamEncoder(lib, w, h, cqm, batch=B, n_frames=N, ...)
        enc.run(fill, on_launch)      # codes N frames of every chain; on_launch(coded, stream) after every launch (e.g. to enqueue a
                                      # payload copy behind it: a chain's payload buffer is reused by its next frame)

    fill(picture, frame) is StreamEncoder.step's: enc.src_ctx.upload per chain, or enc.src_ctx.import_surfaces(picture, surfaces) once for the chains
    whose pictures already lie in device memory (frame.CSP_I420 / CSP_YV12 / CSP_NV12, optionally | CSP_VFLIP) -- asynchronous on the lookahead's stream.
    """

    def __init__(self, lib, width, height, cqm, batch=1, n_frames=None, drift=2, launches=8, **kw):
        if n_frames is None:
            raise ValueError("AsyncStreamEncoder: n_frames (pictures per chain) is needed")
        if kw.get("noise_reduction"):
            raise ValueError("AsyncStreamEncoder: --nr: a launch's B kernel ends on a stream of its own, and a chain's noise-reduction sums must be "
                             "complete before its update (x264hip_noise_reduction_update_chains) and the update before the chain's next sweep: that "
                             "ordering is not built here; StreamEncoder and ChainEncoder code --nr")
        if kw.get("inter", 0) & 0x20 and kw.get("subme", 0) >= 6:
            raise ValueError("AsyncStreamEncoder: sub-8x8 partitions (inter & 0x20) with the RD levels (subme >= 6): the chain's record of cache leftovers "
                             "(x264hip_slice_rd.mb_carry) must pass from each sweep of a chain to the next in coding order, and launches of different "
                             "ages overlap here; StreamEncoder and ChainEncoder code it")
        bf = kw.get("bframes", 0)
        b_adapt = kw.get("b_adapt", 1)
        delay = (max(bf, 3) * 4 if b_adapt == 2 and bf else bf)
        kw.setdefault("n_slots", delay + bf + 3 + drift)
        super().__init__(lib, width, height, cqm, batch=batch, n_frames=None, lookahead_priority=True, **kw)
        from .frame import FrameCtx
        self.total, self.delay, self.drift = n_frames, delay, drift
        B = batch
        tb = lib.x264hip_chain_sweep_bytes()
        self.lctx = []
        for _ in range(launches):
            lc = FrameCtx(lib, width, height, batch=B)
            # (element lists in pinned host memory, read by the filter kernels in place: with the device kept full, even a tiny upload's copy
            # kernel would wait for a wave slot)
            self.lctx.append(dict(ctx=lc, tab_host=lib.x264hip_host_alloc(tb * B), tab_dev=DeviceArray(lib, (tb * B,), np.uint8),
                                  elems=[lib.x264hip_host_alloc(4 * B) for _ in range(len(self.pool))],
                                  ev_ip=lib.x264hip_event_create(), ev_b=lib.x264hip_event_create(), busy=False, ip=[], b=[], keep=None))
        # a chain's next frame may be launched while the copy of its previous payload is still queued: two sets of what a frame writes
        d = self.ctx.dims
        alt = self._frame_bufs(B, d.mb_w * d.mb_h, self.payload_cap, 0)
        self.rd_bufs_alt = dict(self.rd_bufs, **alt)
        self._alt_only = alt
        self.las = self.lb.chains                        # one host state machine per chain (the batch object's lock-step driver is not used)
        self.fed = [0] * B
        self.ncoded = [0] * B
        self.inflight_frame = [-1] * B
        self.prepared = 0                                # pictures prepared on the device (for all chains)
        self.n_launches = 0
        self.launch_sizes = []
        self.pic_events = {}                             # per picture number: what says "in place" to the sweeps that read it (_prepare_picture)
        self.coded_all = [[] for _ in range(B)]          # per chain: the Coded records of its frames, in coding order
        self.next_frame, self.cost_batches, self.undecided = {}, [], set()
        if self.quality is not None:
            raise ValueError("AsyncStreamEncoder: psnr / ssim: a launch's B kernel ends on a stream of its own and its chains move on at once; the quality "
                             "pass is enqueued per step (StreamEncoder) or per frame (ChainEncoder)")
        if self.cavlc:
            raise ValueError("AsyncStreamEncoder: cabac=0: the CAVLC pass follows a step's whole sweep on one stream (StreamEncoder); here a launch's B kernel "
                             "ends on a stream of its own")
        if self.post_scenecut:
            raise ValueError("AsyncStreamEncoder: the post-encode scene cut's check is made per step (StreamEncoder); run with pre_scenecut=1")
        if self.direct_auto:
            raise ValueError("AsyncStreamEncoder: --direct auto's running scores are kept per step (StreamEncoder)")

    def _bufs_of(self, ci):
        return self.rd_bufs_alt if self.c_coded[ci] & 1 else self.rd_bufs

    def payload_bufs(self, cd_index, ci):
        """The buffer set chain ci's frame number cd_index (0-based, coding order) was written to."""
        return self.rd_bufs_alt if cd_index & 1 else self.rd_bufs

    def payload_async_of(self, cd, index, c, ev_b, host_len, host_buf, nbytes):
        """From on_launch: enqueue, behind the frame `cd` (its chain's frame number `index`) of the launch on context c, the copy of its payload
        length and first nbytes payload bytes into pinned host memory; valid once c's stream has passed this point (run() returns after that)."""
        from .slice import PAYLOAD_LEAD
        rb = self.payload_bufs(index, cd.chain)
        st = c.stream
        if cd.slice_type == SLICE_B:                     # the B kernel runs on the library's second stream of this context
            self.lib.x264hip_stream_wait_event(st, ev_b)
        self.lib.x264hip_memcpy_d2h_async(host_len, rb["payload_len"].ptr + 4 * cd.chain, 4, st)
        self.lib.x264hip_memcpy_d2h_async(host_buf, rb["payload"].ptr + self.payload_cap * cd.chain + PAYLOAD_LEAD, nbytes, st)

    # -- pictures --------------------------------------------------------------------------------------------------------------------
    def _oldest_needed(self):
        m = self.prepared
        for ci, la in enumerate(self.las):
            if self.inflight_frame[ci] >= 0:
                m = min(m, self.inflight_frame[ci])
            if self.ncoded[ci] + (1 if self.inflight_frame[ci] >= 0 else 0) < self.total:
                m = min(m, la.oldest_live() if self.fed[ci] else 0)
        return m

    def _prepare_picture(self, fill):
        """Picture number self.prepared for every chain: source, lowres planes, intra costs, AQ offsets.  False: its slot is still in use."""
        f = self.prepared
        if f >= self.total or f - self._oldest >= self.n_slots:
            return False
        pic = self.look.begin_frame(f)
        self._fill(fill, pic, f)
        self.look.prepare(f)
        # what says "picture f is in place" to the sweeps that will read it (they run on other streams)
        ev = self.pic_events.pop(f - self.n_slots, None) or self.lib.x264hip_event_create()
        self.lib.x264hip_event_record(ev, self.src_ctx.stream)
        self.pic_events[f] = ev
        self.prepared += 1
        return True

    # -- the scheduler ---------------------------------------------------------------------------------------------------------------
    def _decide(self, chains, fill):
        """The lookahead's part for `chains` (idle, or with a frame in flight -- the decision does not read its result): pictures in, queues
        asked.  A chain ends up with its next frame in self.next_frame, or pending on a batch of cost tasks launched here (not waited for), or
        back in self.undecided (no slot free for a picture / no launch buffer free)."""
        tasks, specs, owners = [], [], []
        for ci in chains:
            if self.ncoded[ci] + (1 if self.inflight_frame[ci] >= 0 else 0) >= self.total or ci in self.next_frame:
                continue
            want = min(self.total, self.ncoded[ci] + (1 if self.inflight_frame[ci] >= 0 else 0) + self.delay + 1)
            ok = True
            while self.fed[ci] < want:
                if self.fed[ci] >= self.prepared and not self._prepare_picture(fill):
                    ok = False                           # the ring is full: this chain is too far ahead of the slowest one, it waits
                    break
                assert self.las[ci].put() == self.fed[ci]
                self.fed[ci] += 1
            if not ok:
                self.undecided.add(ci)
                continue
            kind, fr, needs = self.las[ci].get(self.fed[ci] >= self.total, self.lb.speculative)
            if kind == LA.FRAME:
                self.next_frame[ci] = fr
            elif kind == LA.NEED:
                if len(tasks) + len(needs) > self.look.max_tasks:
                    self.undecided.add(ci)
                    continue
                for (b, p0, p1, ds0, ds1, spec) in needs:
                    tasks.append((ci, b, p0, p1, ds0, ds1)); specs.append(spec)
                owners.append(ci)
            elif kind != LA.END:
                raise RuntimeError("AsyncStreamEncoder: chain %d has no frame although %d pictures are in" % (ci, self.fed[ci]))
        if tasks:
            h = self.look.run_async(tasks)
            if h is None:                                # every launch buffer is in flight: ask again later
                self.undecided.update(owners)
            else:
                self.lb.rounds += 1
                self.cost_batches.append((h, tasks, specs, owners))

    def run(self, fill, on_launch=None, until=None, poll_s=0.001):
        """Code frames until every chain has coded `until` of them (default: all n_frames), then wait for the device.  May be called again with a
        larger `until` (a benchmark's warm-up, then its timed part)."""
        import time
        L, B = self.lib, self.ctx.batch
        target = self.total if until is None else min(until, self.total)
        idle = {ci for ci in range(B) if self.inflight_frame[ci] < 0}           # chains whose previous frame (if any) is done
        done = sum(1 for ci in range(B) if self.ncoded[ci] >= target)
        self._oldest = self._oldest_needed()
        self._decide([ci for ci in sorted(idle) if self.ncoded[ci] < target], fill)
        stats = os.environ.get("X264HIP_ASYNC_STATS")
        t_last, acc = time.perf_counter(), [0.0, 0.0, 0.0, 0.0, 0.0]
        while done < B:
            progressed = False
            if stats:                                    # time-weighted: idle chains, idle chains without a decision, launches in flight, cost batches in flight
                now = time.perf_counter(); dt_ = now - t_last; t_last = now
                n_idle = sum(1 for ci in idle if self.ncoded[ci] < target)
                acc[0] += dt_; acc[1] += dt_ * n_idle; acc[2] += dt_ * sum(1 for ci in idle if self.ncoded[ci] < target and ci not in self.next_frame)
                acc[3] += dt_ * sum(1 for lc in self.lctx if lc["busy"]); acc[4] += dt_ * len(self.cost_batches)
            # 1. sweeps: the B kernel and the I / P kernel (+ its filters) of every launch in flight, separately
            for lc in self.lctx:
                if not lc["busy"]:
                    continue
                for kind in ("b", "ip"):
                    if lc[kind] and L.x264hip_event_query(lc["ev_" + kind]) == 1:
                        for ci in lc[kind]:
                            self.inflight_frame[ci] = -1
                            self.ncoded[ci] += 1
                            if self.ncoded[ci] == target:
                                done += 1
                        idle.update(lc[kind]); lc[kind] = []; progressed = True
                if not lc["b"] and not lc["ip"]:
                    lc["busy"], lc["keep"] = False, None
            # 2. cost batches: results in, the chains that asked go on deciding
            if self.cost_batches:
                keep_b, again = [], []
                for (h, tasks, specs, owners) in self.cost_batches:
                    res = self.look.poll(h)
                    if res is None:
                        keep_b.append((h, tasks, specs, owners))
                        continue
                    for (ci, b, p0, p1, ds0, ds1), spec, r in zip(tasks, specs, res):
                        self.las[ci].set_cost(b, p0, p1, int(r[0]), int(r[1]), int(r[2]), spec)
                    again += owners
                    progressed = True
                self.cost_batches = keep_b
                if again:
                    self._oldest = self._oldest_needed()
                    self._decide(again, fill)
            if self.undecided and progressed:
                again, self.undecided = sorted(self.undecided), set()
                self._oldest = self._oldest_needed()
                self._decide(again, fill)
            # 3. launch: idle chains whose next frame is decided
            free = [lc for lc in self.lctx if not lc["busy"]]
            go = [ci for ci in idle if ci in self.next_frame and self.ncoded[ci] < target] if free else []
            if not go:
                if not progressed:
                    time.sleep(poll_s)
                continue
            lc = free[0]
            c = lc["ctx"]
            pairs = [(ci, self.next_frame.pop(ci)) for ci in sorted(go)]
            for ci, fr in pairs:
                self.inflight_frame[ci] = fr.frame
                idle.discard(ci)

            def publish(pic_i, chains):                  # the launch's own list for that picture, in pinned host memory
                np.ctypeslib.as_array(C.cast(lc["elems"][pic_i], C.POINTER(C.c_int32)), (B,))[:len(chains)] = chains
                return lc["elems"][pic_i]

            def wait_pictures():
                # the pictures these sweeps read were prepared on the lookahead's stream: wait (on the device) for the ones that may not be finished
                for f in {fr.frame for _, fr in pairs}:
                    ev = self.pic_events.get(f)
                    if ev is not None and L.x264hip_event_query(ev) != 1:
                        L.x264hip_stream_wait_event(c.stream, ev)

            out, keep, filt, ev = self._launch(c, pairs, lc["tab_host"], lc["tab_dev"].p, publish, wait_pictures, (lc["ev_ip"], lc["ev_b"]))
            for cd in out:
                self.coded_all[cd.chain].append(cd)
            if ev:
                px = self.ctx.dims.mb_w * 16 * self.ctx.dims.lines_y
                self.sweep_events.append((ev[0], ev[1], sum(1 for cd in out if cd.slice_type != SLICE_B), sum(px * (3.0 + 4.5 * (cd.n_ref0 + cd.n_ref1)) for cd in out if cd.slice_type != SLICE_B), "IP"))
            self.last_ctx = c
            if on_launch is not None:
                on_launch(out, c, lc["ev_b"])            # e.g. copies of the payloads just produced (a B chain's: behind ev_b)
            # the kept frames' chains are free when the filters are done: the event that says so is recorded behind them
            L.x264hip_event_record(lc["ev_ip"], c.stream)
            lc["busy"], lc["keep"] = True, keep
            lc["ip"] = [cd.chain for cd in out if cd.slice_type != SLICE_B]
            lc["b"] = [cd.chain for cd in out if cd.slice_type == SLICE_B]
            launched = [cd.chain for cd in out]
            for ci in launched:
                self.las[ci].end()
            self.n_launches += 1
            self.launch_sizes.append(len(out))
            # their next decisions now, beside the sweeps (x264_ratecontrol_start does not read what the frame in flight produces)
            self._oldest = self._oldest_needed()
            self._decide(launched, fill)
        if stats and acc[0] > 0:
            print("async stats: %.1f s, mean idle chains %.0f (undecided %.0f) of %d, launches in flight %.1f, cost batches in flight %.1f, launches %d"
                  % (acc[0], acc[1] / acc[0], acc[2] / acc[0], B, acc[3] / acc[0], acc[4] / acc[0], self.n_launches), file=sys.stderr)
        for lc in self.lctx:
            lc["ctx"].sync()
        assert self.lib.x264hip_device_synchronize() == 0

    def status(self):
        super().status()
        for lc in self.lctx:
            for s in self.states:
                lc["ctx"].check(self.lib.x264hip_slice_sweep_status(lc["ctx"].h, C.byref(s.st)), "slice_sweep_status")

    def close(self):
        assert self.lib.x264hip_device_synchronize() == 0
        for a in self._alt_only.values():
            a.free()
        for lc in self.lctx:
            lc["tab_dev"].free()
            for hp in [lc["tab_host"]] + lc["elems"]:
                self.lib.x264hip_host_free(hp)
            for e in (lc["ev_ip"], lc["ev_b"]):
                self.lib.x264hip_event_destroy(e)
            lc["ctx"].close()
        self.lctx = []
        super().close()
