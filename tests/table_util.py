"""Helper of the chain-table tests (tests/test_gpu_lossless_raster.py, tests/test_gpu_edge_table.py): a batch of I / P chains through
x264hip_slice_sweep_chains, every chain with its own constant QP and, if wanted, its own clip.  StreamEncoder is the product's caller of
that entry point; it cannot reach it on pictures the lookahead refuses (mb_w <= 2 or mb_h <= 2), this helper can."""
import ctypes as C

import numpy as np

from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.frame import DeviceArray
from x264_vs2008_amd.stream import ChainSweep


def table_launch(hip_lib, cqm, size, frames, y, u, v, kw, qps, clips=None, arrays=("mb_type",)):
    """Every frame of a batch of len(qps) chains through x264hip_slice_sweep_chains, chain b at constant QP qps[b] (its I slices at the QP
    that constant gives I slices: slice.iframe_qp) on clips[b] = (y, u, v) -- without clips every chain is fed y, u, v: one ChainEncoder
    per QP value owns the tables of its chains, all of them share the first one's context, pictures and states.  kw: ChainEncoder's
    options.  Returns per frame the payloads of every chain, mb_bits, the state arrays named in `arrays` (mb_type also under its own
    key), the planes before (rec) and behind (fin) the frame-end filters; raises what the library refuses."""
    B = len(qps)
    if clips is None:
        clips = [(y, u, v)] * B
    encs = {}
    for q in sorted(set(qps)):
        encs[q] = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, batch=B, write=1, **dict(kw, qp=q))
    e0 = encs[qps[0]]
    lib, c = hip_lib, e0.ctx
    aq = e0.rd_opt["aq_mode"]
    tb = lib.x264hip_chain_sweep_bytes()
    tab_host = lib.x264hip_host_alloc(tb * B)
    tab_dev = DeviceArray(lib, (tb * B,), np.uint8)
    out = []
    try:
        for f in range(frames):
            for b in range(B):
                e0.upload(clips[b][0][f], clips[b][1][f], clips[b][2][f], b=b)
            idr = f == 0
            stype = sl.SLICE_I if idr else sl.SLICE_P
            if idr:
                e0.refs = []
            used = [r[0] for r in e0.refs]
            pic_i = next(i for i, p in enumerate(e0.pool) if not any(p is q for q in used))
            recon, state = e0.pool[pic_i], e0.states[pic_i]
            refs, _ = e0.ref_lists(e0.refs, 2 * f, stype)
            arr = (C.c_void_p * max(len(refs), 1))(*[C.addressof(r[0]) for r in refs]) if refs else None
            if aq:                             # x264_adaptive_quant_frame on every chain's source: [batch][n_mb] offsets, the kernel adds the chain's
                c.check(lib.x264hip_adaptive_quant_frame(c.h, C.byref(e0.fenc), e0.rd_opt["aq_strength"], e0.rd_bufs["aq_energy"].p, e0.rd_bufs["aq_offset"].p),
                        "adaptive_quant_frame")
            entries, keep = (ChainSweep * B)(), []
            for b in range(B):
                e = encs[qps[b]]
                qp = sl.iframe_qp(qps[b]) if idr else qps[b]
                p = e.slice_params(stype, qp, 2 * f, e.cost_table(qp).ptr, None)
                rd = e.slice_rd(dict(e.rd_bufs, payload=e0.rd_bufs["payload"], payload_len=e0.rd_bufs["payload_len"], mb_bits=e0.rd_bufs["mb_bits"],
                                     stale=e0.rd_bufs["stale"]), float(qp), e0.i_frame, e0.rd_bufs["aq_offset"].ptr if aq else None, 1, 0)      # (i_frame: x264_cabac_encode_flush's padding bit)
                rd.payload_cap = e0.payload_cap
                p.rd = C.addressof(rd)
                for i, r in enumerate(refs):
                    p.ref_poc[i] = r[2]
                keep += [p, rd]
                entries[b] = ChainSweep(chain=b, fenc=C.addressof(e0.fenc), refs=C.cast(arr, C.c_void_p) if arr else None, n_refs=len(refs),
                                        recon=C.addressof(recon), params=C.addressof(p), l0=C.addressof(refs[0][1].st) if refs else None, out=C.addressof(state.st))
            c.check(lib.x264hip_mb_state_clear_progress(c.h, C.byref(state.st)), "mb_state_clear_progress")
            c.check(lib.x264hip_slice_sweep_chains(c.h, entries, B, tab_host, tab_dev.p), "slice_sweep_chains")
            e0.last, e0.last_ctx, e0.last_bufs, e0.last_is_b, e0.last_poc = (recon, state), c, e0.rd_bufs, False, 2 * f
            e0.status()
            rec = [np.stack([c.download(recon, nm, padded=False, b=b) for b in range(B)]) for nm in ("y", "u", "v")]
            d = dict(payload=e0.payloads(), rec=rec, mb_bits=e0.rd_bufs["mb_bits"].get(), state={k: state.get(k) for k in arrays})
            d["mb_type"] = d["state"]["mb_type"]
            e0.finish_frame()
            c.sync()
            d["fin"] = [np.stack([c.download(recon, nm, padded=False, b=b) for b in range(B)]) for nm in ("y", "u", "v")]
            out.append(d)
    finally:
        c.sync()
        tab_dev.free()
        lib.x264hip_host_free(tab_host)
        for e in encs.values():
            e.close()
    return out
