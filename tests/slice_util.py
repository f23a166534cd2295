"""Helpers of the macroblock-sweep parity tests: run a chain through the ChainEncoder -- the wavefront variant (run_chain) or the
raster-order variant with its entropy coder (run_chain2) -- and download, per frame, what the reference's loop is compared on;
check_frame holds one frame of one chain to a golden chain (tests/golden/slice_*.npz, slice2_*.npz)."""
import ctypes as C
import os

import numpy as np

from paths import GOLDEN
from x264_vs2008_amd import slice as sl

STATE = ["mb_type", "partition", "sub_partition", "ref", "i4mode", "i16mode", "chroma_mode", "qp", "t8", "mv", "cbp", "nnz", "luma", "luma_dc",
         "chroma_dc", "chroma_ac"]


def run_chain(hip_lib, cqm, size, frames, y, u, v, kw, batch=1, shift=0):
    """Encode the clip; returns per frame a dict of downloaded arrays (batch element 0 unless stated)."""
    kw = dict(kw)
    if kw.pop("cqm_preset", 0):                      # --cqm jvt: the quantiser tables x264_cqm_init builds for the JVT matrices
        with np.load(os.path.join(GOLDEN, "cqm_jvt.npz")) as z:
            cqm = {k: z[k] for k in z.files}
    enc = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, batch=batch, **kw)
    out = []
    try:
        for f in range(frames):
            for b in range(batch):
                t = (f + b * shift) % frames if shift else f
                enc.upload(y[t], u[t], v[t], b=b)
            stype, qp, state = enc.encode_frame()
            enc.status()
            recon = enc.last[0]
            d = {k: state.get(k) for k in STATE + ["mvr", "cost_intra", "cost_inter"]}
            d["info"] = (stype, qp)
            for nm in ("y", "u", "v"):
                d["rec_" + nm] = np.stack([enc.ctx.download(recon, nm, padded=False, b=b) for b in range(batch)])
            enc.finish_frame()
            enc.ctx.sync()
            for nm in ("y", "u", "v"):
                d["fin_" + nm] = np.stack([enc.ctx.download(recon, nm, padded=False, b=b) for b in range(batch)])
            out.append(d)
    finally:
        enc.close()
    return out


def check_frame(d, gold, f, n_refs, b=0):
    for k in STATE:
        got, want = d[k][b], gold[k][f]
        assert np.array_equal(got.reshape(want.shape), want), "frame %d: %s differs first at %s" % (f, k, np.argwhere(got.reshape(want.shape) != want)[:3].tolist())
    for nm in ("y", "u", "v"):
        for kind in ("rec_", "fin_"):
            got, want = d[kind + nm][b], gold[kind + nm][f]
            assert np.array_equal(got, want), "frame %d: %s%s differs at %s" % (f, kind, nm, np.argwhere(got != want)[:3].tolist())
    skip = gold["mb_type"][f] == sl.P_SKIP
    nr = int(gold["frame_info"][f][2])
    for r in range(nr):
        got, want = d["mvr"][b][r], gold["mvr"][f][r]
        assert np.array_equal(got[~skip], want[~skip]), "frame %d: mvr[%d]" % (f, r)
    assert d["info"] == (int(gold["frame_info"][f][0]), int(gold["frame_info"][f][1])), "frame %d: (slice type, QP) %s, the reference %s" % (f, d["info"], gold["frame_info"][f][:2].tolist())
    assert int(d["cost_intra"][b].sum()) == int(gold["stat"][f][0]) and int(d["cost_inter"][b].sum()) == int(gold["stat"][f][1]), "frame %d: intra / inter cost sums" % f


def lowres_arrays(hip_lib, seed, frames, size, batch=1):
    """The fixture's stand-in lookahead vectors (oracle/refslice.py: lowres_vectors) on the device: [(list 0, list 1)] per frame in coding order."""
    if seed is None:
        return None
    from oracle.refslice import lowres_vectors
    from x264_vs2008_amd.frame import DeviceArray
    n = ((size[0] + 15) // 16) * ((size[1] + 15) // 16)
    lm = lowres_vectors(seed, frames, n)
    return [tuple(DeviceArray(hip_lib, (batch, n, 2), np.int16, np.ascontiguousarray(np.broadcast_to(lm[f, l], (batch, n, 2)))) for l in range(2)) for f in range(frames)]


def run_chain2(hip_lib, cqm, size, frames, y, u, v, kw, ekw, batch=1):
    kw = dict(kw)
    kw.pop("cqm_preset", 0)
    ekw = dict(ekw)
    lowres = lowres_arrays(hip_lib, ekw.pop("lowres_seed", None), frames, size, batch)
    enc = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, batch=batch, write=1, **kw, **{k: v_ for k, v_ in ekw.items() if k != "write"})
    out = []
    # B frames: the chain in coding order (the golden fixtures of such chains are in coding order too)
    order = sl.coding_order(frames, kw.get("keyint", 0), ekw["bframes"]) if ekw.get("bframes") else None
    try:
        for f in range(frames):
            disp = order[f][0] if order else f
            for b in range(batch):
                enc.upload(y[disp], u[disp], v[disp], b=b)
            lw = dict(lowres_mv=lowres[f][0], lowres_mv1=lowres[f][1]) if lowres else {}
            stype, qp, state = enc.encode_frame(stype=order[f][1], disp=disp, **lw) if order else enc.encode_frame(**lw)
            enc.status()
            recon = enc.last[0]
            d = {k: state.get(k) for k in STATE + ["mvr", "cost_intra", "cost_inter"]}
            if order:
                n_mb = state.get("mb_type").shape[1]
                for nm, tail, dt in (("mv1", (16, 2), np.int16), ("ref1", (4,), np.int8)):
                    a = np.zeros((batch, n_mb) + tail, dt)
                    assert enc.ctx.lib.x264hip_memcpy_d2h(a.ctypes.data_as(C.c_void_p), getattr(state.st, nm), a.nbytes) == 0, "frame %d: copying %s from the device failed" % (f, nm)
                    if stype != sl.SLICE_B:               # the reference reports zeros / -1 outside B slices
                        a[...] = 0 if nm == "mv1" else -1
                    d[nm] = a
            d["info"] = (stype, qp)
            d["payload"] = enc.payloads()
            d["mb_bits"] = enc.rd_bufs["mb_bits"].get()
            for nm in ("y", "u", "v"):
                d["rec_" + nm] = np.stack([enc.ctx.download(recon, nm, padded=False, b=b) for b in range(batch)])
            enc.finish_frame()
            enc.ctx.sync()
            for nm in ("y", "u", "v"):
                d["fin_" + nm] = np.stack([enc.ctx.download(recon, nm, padded=False, b=b) for b in range(batch)])
            out.append(d)
    finally:
        enc.close()
    return out
