"""GPU: what a frame context owns lives and dies with it.  The second stream and the two events of a chain-table launch that runs its B kernel
beside its I / P kernels belong to the x264hip_frame_ctx: x264hip_frame_ctx_delete releases them (a caller's stream, handed in through
x264hip_frame_ctx_set_b_stream, stays the caller's), and a context created later -- often at the address the deleted one had -- starts with
none.  Encoders opened and closed one after another in one process, and two contexts of one geometry one after the other around the death
of the first one's B stream, must code what the reference codes."""
import ctypes as C
import os

import numpy as np
import pytest

import stream_util as ts
from conftest import GOLDEN
from oracle import refslice as rs
from x264_vs2008_amd import lib as L
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.frame import DeviceArray, FrameCtx
from x264_vs2008_amd.stream import ChainSweep

pytestmark = pytest.mark.gpu


def test_stream_encoders_one_after_another_equal_reference_fixture(hip_lib):
    """The fixture's first two chains (clips of their own, so their B frames fall on different steps) through three StreamEncoders, each
    closed before the next is opened: every run's frame order, types, QPs and payload bytes are the reference's, and steps that code a B chain
    and an I / P chain in one launch -- the two-stream path -- did occur."""
    name = "badapt1_crf_aq"
    cs = ts.chains(name, ts.SEEDS[name][:2])
    with np.load(os.path.join(GOLDEN, "stream_%s.npz" % name)) as z:
        gold = [{k: z["c%d_%s" % (i, k)] for k in ("frame_info", "frame_info2", "payload", "payload_len")} for i in range(len(cs))]
    frames = cs[0]["frames"]
    clips = [ts.K.clip(c["w"], c["h"], frames, c["cut"], c["t0"], c["slow"]) for c in cs]
    for run in range(3):
        enc = ts.encoder_for(hip_lib, cs[0], len(cs))
        got, mixed = [[] for _ in cs], 0

        def fill(pic, f):
            for b, (y, u, v) in enumerate(clips):
                enc.src_ctx.upload(pic, y[f], u[f], v[f], b=b)

        try:
            fed, idle = 0, 0
            for _ in range(4 * frames + 40):
                coded = enc.step(fill if fed < frames else None)
                fed += fed < frames
                idle = 0 if coded else idle + (fed >= frames and enc.flushing)
                if idle >= 2:
                    break
                if coded:
                    enc.sync()
                    enc.status()
                    pl = enc.payloads()
                    for cd in coded:
                        got[cd.chain].append((cd.frame, cd.slice_type, cd.qp, pl[cd.chain]))
                    mixed += len({cd.slice_type == sl.SLICE_B for cd in coded}) == 2
        finally:
            enc.close()
        for i, c in enumerate(cs):
            ts.check(got[i], gold[i], c, "run %d chain %d" % (run, i))
        assert mixed >= 1, "run %d: no step coded a B chain beside an I / P chain: the two-stream path did not run" % run


def test_context_after_one_whose_b_stream_died_equals_reference(hip_lib, oracle_lib, cqm):
    """The smallest chain-table launch on two streams: chain 0 codes the P frame, chain 1 the B frame of an I P B P chain (coding order) of
    80x64.  Context A runs it with a caller's B stream, is deleted, the stream is destroyed; context B, of the same geometry, runs it again.
    Both give the bytes and decisions of the reference loop's twin for those two frames, and neither leaves an error or an abort behind."""
    lib = hip_lib
    w, h, n = 80, 64, 4
    kw = dict(qp=26, subme=5, me_method=1, n_refs=2, inter=0x113, intra=0x3, transform8x8=1, cabac=1, deblock=1)
    ekw = dict(bframes=1, weightb=1, direct_pred=1)
    # (the synthetic clip's moving box needs pictures above 64x64: the top left 80x64 of a 96x80 clip)
    y, u, v = (np.ascontiguousarray(a[:, :h >> s, :w >> s]) for a, s in zip(rs.clip(96, 80, n), (0, 1, 1)))
    want = rs.run2(oracle_lib, "x264o_encode_chain2", rs.make_params(w, h, n, **kw), rs.make_ext(**ekw), y, u, v)
    order = sl.coding_order(n, 0, 1)
    assert order == [(0, sl.SLICE_I), (2, sl.SLICE_P), (1, sl.SLICE_B), (3, sl.SLICE_P)]
    assert (want["mb_type"][2] >= 7).any()                 # B macroblock types (B_DIRECT ..) in the B frame
    cfg = L.Cfg(int(os.environ.get("LOCAL_RANK", "0")), 0)
    assert lib.x264hip_init(C.byref(cfg)) == 0              # (the only call that clears the error text earlier tests may have left)
    assert lib.x264hip_last_error() == b""
    enc = sl.ChainEncoder(lib, w, h, cqm, batch=2, write=1, **kw, **ekw)
    tb = lib.x264hip_chain_sweep_bytes()
    tab_host = lib.x264hip_host_alloc(tb * 2)
    tab_dev = DeviceArray(lib, (tb * 2,), np.uint8)
    stream = ctx = None
    try:
        for disp, stype in order[:2]:                        # I0 and P2 of both chains in lock step: the pictures the launch predicts from
            for b in range(2):
                enc.upload(y[disp], u[disp], v[disp], b=b)
            enc.encode_frame(stype=stype, disp=disp)
            enc.status()
            enc.finish_frame()
        for b, disp in enumerate((3, 1)):
            enc.upload(y[disp], u[disp], v[disp], b=b)
        enc.ctx.sync()
        used = [r[0] for r in enc.refs]
        pic_i = next(i for i, p in enumerate(enc.pool) if not any(p is q for q in used))
        recon, state = enc.pool[pic_i], enc.states[pic_i]
        entries, keep = (ChainSweep * 2)(), []
        for b, (stype, disp, i_frame) in enumerate(((sl.SLICE_P, 3, 3), (sl.SLICE_B, 1, 2))):
            refs, refs1 = enc.ref_lists(enc.refs, 2 * disp, stype)
            qp = sl.bframe_qp(kw["qp"]) if stype == sl.SLICE_B else kw["qp"]
            p = enc.slice_params(stype, qp, 2 * disp, enc.cost_table(qp).ptr, None)
            rd = enc.slice_rd(enc.rd_bufs, float(qp), i_frame, None, 1, 0)
            p.rd = C.addressof(rd)
            if stype == sl.SLICE_B:
                sb = sl.SliceB(fref1=C.addressof(refs1[0][0]), l1_state=C.addressof(refs1[0][1].st), ref1_poc=refs1[0][2], weightb=1, direct_spatial=1)
                p.b = C.addressof(sb)
                keep.append(sb)
            for i, r in enumerate(refs):
                p.ref_poc[i] = r[2]
            arr = (C.c_void_p * len(refs))(*[C.addressof(r[0]) for r in refs])
            out = sl.MbState.from_buffer_copy(state.st)     # every chain its own copy of the structure: the same arrays, its own scalars
            keep += [p, rd, arr, out]
            entries[b] = ChainSweep(chain=b, fenc=C.addressof(enc.fenc), refs=C.cast(arr, C.c_void_p), n_refs=len(refs), recon=C.addressof(recon),
                                    params=C.addressof(p), l0=C.addressof(refs[0][1].st), out=C.addressof(out))

        def launch(c):
            c.check(lib.x264hip_mb_state_clear_progress(c.h, C.byref(state.st)), "mb_state_clear_progress")
            c.check(lib.x264hip_slice_sweep_chains(c.h, entries, 2, tab_host, tab_dev.p), "slice_sweep_chains")
            c.sync()
            assert lib.x264hip_slice_sweep_status(c.h, C.byref(state.st)) == 0, lib.x264hip_last_error()
            got = {k: state.get(k) for k in ("mb_type", "mv", "ref", "cbp", "qp")}
            got["payload"] = enc.payloads()
            return got

        stream = lib.x264hip_stream_create()
        assert stream
        ctx = FrameCtx(lib, w, h, batch=2)                   # context A
        ctx.check(lib.x264hip_frame_ctx_set_b_stream(ctx.h, stream), "frame_ctx_set_b_stream")
        got_a = launch(ctx)
        ctx.close()                                          # x264hip_frame_ctx_delete
        ctx = None
        lib.x264hip_stream_destroy(stream)
        stream = None
        ctx = FrameCtx(lib, w, h, batch=2)                   # context B: the library's own B stream, made by this launch
        got_b = launch(ctx)
        ctx.close()                                          # x264hip_frame_ctx_delete
        ctx = None
        assert lib.x264hip_last_error() == b""
    finally:
        if ctx is not None:
            ctx.close()
        if stream:
            lib.x264hip_stream_destroy(stream)
        tab_dev.free()
        lib.x264hip_host_free(tab_host)
        enc.close()
    for what, got in (("context A", got_a), ("context B", got_b)):
        for b, f in enumerate((3, 2)):                       # chain 0: the reference's coded frame 3 (P3); chain 1: its coded frame 2 (B1)
            assert got["payload"][b] == bytes(want["payload"][f, :want["payload_len"][f]]), "%s chain %d: payload differs from the reference loop's" % (what, b)
            for k in ("mb_type", "mv", "ref", "cbp", "qp"):
                assert np.array_equal(got[k][b].reshape(want[k][f].shape), want[k][f]), "%s chain %d: %s differs from the reference loop's" % (what, b, k)
    for k in got_a:
        assert np.array_equal(got_a[k], got_b[k]) if k != "payload" else got_a[k] == got_b[k], "context B's %s differs from context A's" % k
