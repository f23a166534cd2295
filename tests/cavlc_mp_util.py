"""Helpers of tests/test_gpu_cavlc_mp.py: chains through ChainEncoder and StreamEncoder with the serial CAVLC pass or the macroblock-parallel
one (cavlc_mp), keeping what the two must agree on -- payload bytes, payload_len and mb_bits of every chain and frame -- and the comparison."""
import numpy as np

import look_cases as K
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.stream import StreamEncoder

P_SKIP = 6


def run_lockstep(lib, cqm, size, clips, order, kw, cavlc_mp):
    """One chain per clip [(y, u, v) with frames first] in lock step; order: [(display index, slice type)] in coding order, or a frame count
    for I / P chains in display order.  Per coded frame: dict(payload=[bytes per chain], payload_len, mb_bits, mb_type)."""
    enc = sl.ChainEncoder(lib, size[0], size[1], cqm, batch=len(clips), write=1, cavlc_mp=cavlc_mp, **kw)
    assert enc.cavlc and enc.cavlc_mp == bool(cavlc_mp)
    out = []
    try:
        for f in range(order if isinstance(order, int) else len(order)):
            disp, stype = (f, None) if isinstance(order, int) else order[f]
            for b, (y, u, v) in enumerate(clips):
                enc.upload(y[disp], u[disp], v[disp], b=b)
            _, _, state = enc.encode_frame() if stype is None else enc.encode_frame(stype=stype, disp=disp)
            enc.status()
            rb = getattr(enc, "last_bufs", None) or enc.rd_bufs
            out.append(dict(payload=enc.payloads(), payload_len=rb["payload_len"].get(), mb_bits=rb["mb_bits"].get(), mb_type=state.get("mb_type")))
            enc.finish_frame()
    finally:
        enc.close()
    return out


def same_frames(got, want, what):
    """The macroblock-parallel pass's frames against the serial pass's."""
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["payload_len"], w["payload_len"]), "%s frame %d: payload_len %s, the serial pass %s" % (what, f, g["payload_len"].tolist(), w["payload_len"].tolist())
        for b in range(len(w["payload"])):
            assert np.array_equal(g["mb_bits"][b], w["mb_bits"][b]), "%s frame %d chain %d: mb_bits differ first at macroblock %d" % (
                what, f, b, np.flatnonzero(g["mb_bits"][b] != w["mb_bits"][b])[0])
            assert g["payload"][b] == w["payload"][b], "%s frame %d chain %d: the payload (%d bytes) differs first at byte %d" % (
                what, f, b, len(w["payload"][b]), next(i for i, (x, z) in enumerate(zip(g["payload"][b], w["payload"][b])) if x != z))


def run_stream(lib, cqm, c, t0s, cavlc_mp):
    """cavlc_b_util.run_cavlc_stream for one chain per entry of t0s (clips that differ, so that the chains' frame types do): per chain, in coding
    order, [(input frame, slice type, qp, payload, payload_len, mb_bits)]."""
    clips = [K.clip(c["w"], c["h"], c["frames"], c["cut"], t0, c["slow"]) for t0 in t0s]
    frames = c["frames"]
    enc = StreamEncoder(lib, c["w"], c["h"], cqm, batch=len(t0s), crf=c["crf"], b_adapt=c["b_adapt"], bframe_bias=c["bframe_bias"], keyint_min=c["keyint_min"],
                        scenecut_threshold=c["scenecut_threshold"], pre_scenecut=c["pre_scenecut"], qp=c["qp"], me_method=c["me"], me_range=16, subme=c["subme"],
                        n_refs=c["n_refs"], inter=c["inter"], intra=0x3, transform8x8=1, cabac=0, deblock=1, keyint=c["keyint"], aq_mode=c["aq"], aq_strength=1.0,
                        bframes=c["bframes"], weightb=c["weightb"], direct_pred=c.get("direct_pred", 1), qp_min=0, cavlc_mp=cavlc_mp)
    got, mixed = [[] for _ in t0s], 0

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
                pl, ln, bits = enc.payloads(), enc.rd_bufs["payload_len"].get(), enc.rd_bufs["mb_bits"].get()
                mixed += len({cd.slice_type for cd in coded}) > 1
                for cd in coded:
                    got[cd.chain].append((cd.frame, cd.slice_type, cd.qp, pl[cd.chain], int(ln[cd.chain]), bits[cd.chain].copy()))
    finally:
        enc.close()
    return got, mixed
