"""Host side of the per-frame measurements (include/x264hip_stream.h: x264hip_frame_report_* on the device, x264hip_stat_* in host C): what x264
core 66 prints per coded frame and when the encoder closes -- PSNR, SSIM, macroblock types, partitions, reference use.

    Reporter   the buffers one context's quality passes write into, and the enqueue itself (lock step: frame(); chain table: chains())
    Stat       x264_encoder_frame_end's sums and x264_encoder_close's report for one stream

The arithmetic lives in the library; this file owns buffers and orders calls."""
import ctypes as C

import numpy as np

from .abi import ChainReport, FrameReport, StatFrame
from .frame import DeviceArray

REPORT_PSNR, REPORT_SSIM, REPORT_REFS = 1, 2, 4
# x264hip_frame_report as a numpy record (abi.FrameReport field by field)
REPORT_DTYPE = np.dtype([("ssd", np.int64, (3,)), ("ssim", np.float64), ("qp_sum", np.int32), ("mb_count", np.int32, (19,)), ("mb_partition", np.int32, (17,)),
                         ("mb_count_8x8dct", np.int32, (2,)), ("mb_count_ref", np.int32, (2, 32)), ("reserved", np.int32)])
assert REPORT_DTYPE.itemsize == C.sizeof(FrameReport)
CHUNK_DTYPE = np.dtype([("ssd", np.uint64, (3,)), ("ssim", np.float32), ("pad", np.int32)])      # the pass's partial results, one per x264_fdec_filter_row call


def flags(psnr, ssim, n_refs):
    return (REPORT_PSNR if psnr else 0) | (REPORT_SSIM if ssim else 0) | (REPORT_REFS if n_refs > 1 else 0)


class Reporter:
    """A ring of `depth` buffer sets for the quality passes of one context, each for up to n_max entries.  A set is reused only after the
    stream has passed its last use (an event per set; the host waits for the stream if it has not), so a caller that enqueues many frames
    between synchronisations stays correct.  The records of an enqueue stay readable until `depth` further enqueues."""

    def __init__(self, ctx, n_max, depth=8):
        L = ctx.lib
        self.ctx, self.lib, self.n_max = ctx, L, n_max
        stage = n_max * max(int(L.x264hip_chain_report_bytes()), int(L.x264hip_frame_report_frame_staging_bytes()))
        self.scratch_per = int(L.x264hip_frame_report_scratch_bytes(ctx.h))
        self.sets, self.i = [], 0
        for _ in range(depth):
            host = L.x264hip_host_alloc(stage)
            if not host:
                raise MemoryError("x264hip_host_alloc(%d)" % stage)
            self.sets.append(dict(host=host, table=DeviceArray(L, (stage,), np.uint8), scratch=DeviceArray(L, (n_max * self.scratch_per,), np.uint8),
                                  out=DeviceArray(L, (n_max * REPORT_DTYPE.itemsize,), np.uint8), ev=None, n=0, keep=None))

    def _next(self, stream):
        s = self.sets[self.i % len(self.sets)]
        self.i += 1
        if s["ev"] is not None and self.lib.x264hip_event_query(s["ev"]) != 1:
            self.lib.x264hip_stream_synchronize(s["stream"])
        return s

    def _done(self, s, stream, n, keep=None):
        if s["ev"] is None:
            s["ev"] = self.lib.x264hip_event_create()
        self.lib.x264hip_event_record(s["ev"], stream)
        s["stream"], s["n"], s["keep"] = stream, n, keep
        return s

    def frame(self, fenc, recon, state, stype, fl):
        """Lock step: every batch element of one source picture, one reconstruction and one state (an MbState), enqueued on the context's stream."""
        c = self.ctx
        s = self._next(c.stream)
        c.check(self.lib.x264hip_frame_report_frame(c.h, C.byref(fenc), C.byref(recon), C.byref(state) if state is not None else None, stype, fl,
                                                    s["host"], s["table"].ptr, s["scratch"].ptr, s["out"].ptr), "frame_report_frame")
        return self._done(s, c.stream, c.batch)

    def chains(self, entries):
        """A chain table: [(chain, fenc, fenc_element, recon, recon_element, state or None, slice type, psnr, ssim, count_refs)] -- pictures and states
        as abi records, kept alive here until the set is reused."""
        c, n = self.ctx, len(entries)
        if n > self.n_max:
            raise ValueError("%d entries, the reporter holds %d" % (n, self.n_max))
        s = self._next(c.stream)
        arr = (ChainReport * n)()
        for i, (chain, fenc, fe, recon, re_, state, stype, psnr, ssim, refs) in enumerate(entries):
            arr[i] = ChainReport(chain=chain, fenc=C.addressof(fenc), fenc_element=fe, recon=C.addressof(recon), recon_element=re_,
                                 state=C.addressof(state) if state is not None else None, slice_type=stype, psnr=int(bool(psnr)), ssim=int(bool(ssim)),
                                 count_refs=int(bool(refs)))
        c.check(self.lib.x264hip_frame_report_chains(c.h, arr, n, s["host"], s["table"].ptr, s["scratch"].ptr, s["out"].ptr), "frame_report_chains")
        return self._done(s, c.stream, n, (arr, entries))

    @staticmethod
    def records(s):
        """The records of one enqueue (valid once its stream has passed it): a numpy record array, REPORT_DTYPE."""
        return s["out"].get()[:s["n"] * REPORT_DTYPE.itemsize].view(REPORT_DTYPE).copy()

    def partials(self, s):
        """The per-call partial results of one enqueue, [entry][mb_h] CHUNK_DTYPE: each x264_fdec_filter_row call's squared errors and SSIM float."""
        per = self.scratch_per // CHUNK_DTYPE.itemsize
        return s["scratch"].get()[:s["n"] * self.scratch_per].view(CHUNK_DTYPE).reshape(s["n"], per).copy()

    def close(self):
        for s in self.sets:
            if s["ev"] is not None:
                self.lib.x264hip_event_destroy(s["ev"])
            self.lib.x264hip_host_free(s["host"])
            for k in ("table", "scratch", "out"):
                s[k].free()
        self.sets = []


class Stat:
    """x264hip_stat: one stream's running statistics.  params: validated abi.EncoderParams."""

    def __init__(self, lib, params, psnr=1, ssim=1):
        self.lib = lib
        self.h = lib.x264hip_stat_new(C.byref(params), int(bool(psnr)), int(bool(ssim)))
        if not self.h:
            raise RuntimeError("x264hip_stat_new failed: %s" % lib.x264hip_last_error().decode())

    def frame_end(self, record, stype, frame_size, nal_ref_idc=0, poc=0, frames_since_ref=0, direct_spatial=1):
        """One coded frame: record = one REPORT_DTYPE element (or an abi.FrameReport).  Returns the X264_LOG_DEBUG line."""
        if not isinstance(record, FrameReport):
            record = FrameReport.from_buffer_copy(np.asarray(record, REPORT_DTYPE).tobytes())
        f = StatFrame(slice_type=stype, frame_size=frame_size, nal_ref_idc=nal_ref_idc, poc=poc, frames_since_ref=frames_since_ref,
                      direct_spatial=direct_spatial)
        line = C.create_string_buffer(256)
        n = self.lib.x264hip_stat_frame_end(self.h, C.byref(f), C.byref(record), line, 256)
        if n < 0:
            raise RuntimeError("x264hip_stat_frame_end failed: %s" % self.lib.x264hip_last_error().decode())
        return line.value.decode()

    @property
    def frames(self):
        return self.lib.x264hip_stat_frames(self.h)

    def summary(self):
        buf = C.create_string_buffer(8192)
        n = self.lib.x264hip_stat_summary(self.h, buf, 8192)
        if n < 0:
            raise RuntimeError("x264hip_stat_summary failed: %s" % self.lib.x264hip_last_error().decode())
        return buf.value.decode()

    def close(self):
        if self.h:
            self.lib.x264hip_stat_delete(self.h)
            self.h = None
