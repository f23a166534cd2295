"""`--no-cabac` with B frames: the raster sweep without its writer, then the CAVLC writer's B-slice syntax (x264hip_cavlc_write_frame for chains
in lock step, x264hip_cavlc_write_chains for chains that are not), against the REFERENCE's own writer inside its macroblock loop
(oracle/ref_slice.c with cabac = 0).  Everything is compared for equality: payload bytes, their length, the bit position after every macroblock.
The configurations, and the check that the reference's decisions reach every branch of the syntax, are in tests/cavlc_b_util.py."""
import ctypes as C
import os

import numpy as np
import pytest

from cavlc_b_util import B_CASES, coverage, reference
from oracle import refslice as rs
from paths import REF_SO
from slice_util import run_chain2
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.frame import DeviceArray, cqm_init
from x264_vs2008_amd.stream import ChainSweep

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs the reference tree)")]


@pytest.mark.parametrize("name", sorted(B_CASES))
def test_cavlc_b_chain_equals_reference(hip_lib, name):
    """ChainEncoder with bframes and cabac = 0: per frame, in coding order, payload_len, the payload bytes and mb_bits are the reference's."""
    size, frames, kind, kw, ekw = B_CASES[name]
    (y, u, v), a = reference(name)
    got = run_chain2(hip_lib, cqm_init(hip_lib), size, frames, y, u, v, kw, ekw)
    assert (a["frame_info"][:, 0] == rs.SLICE_B).sum() >= 3
    for f in range(frames):
        what = "%s coded frame %d (%s)" % (name, f, "PBI"[int(a["frame_info"][f, 0])])
        assert got[f]["info"] == (int(a["frame_info"][f, 0]), int(a["frame_info"][f, 1])), what
        assert np.array_equal(got[f]["mb_type"][0], a["mb_type"][f]), "%s: the sweep without its writer decides differently" % what
        want = bytes(a["payload"][f, :a["payload_len"][f]])
        assert len(got[f]["payload"][0]) == int(a["payload_len"][f]), "%s: payload_len %d, the reference %d" % (what, len(got[f]["payload"][0]), int(a["payload_len"][f]))
        assert got[f]["payload"][0] == want, "%s: payload bytes differ" % what
        assert np.array_equal(got[f]["mb_bits"][0], a["mb_bits"][f]), "%s: mb_bits differ first at macroblock %s" % (what, np.argwhere(got[f]["mb_bits"][0] != a["mb_bits"][f])[:1].tolist())


def test_reference_decisions_reach_every_b_branch():
    """On the REFERENCE's decisions: over the clips of B_CASES every branch of the B syntax occurs, so a later change of inputs cannot
    quietly drop one."""
    total = {}
    for name in B_CASES:
        for k, n in coverage(reference(name)[1]).items():
            total[k] = total.get(k, 0) + n
    missing = [k for k, n in total.items() if n == 0]
    assert not missing, "no macroblock of the reference's runs has: %s" % missing
    # te() with one and with several list-0 references, and list 0 with a single picture (no ref_idx at all)
    n_ref = {int(n) for name in B_CASES for st, n in reference(name)[1]["frame_info"][:, [0, 2]] if st != rs.SLICE_I}
    assert {1, 2, 3} <= n_ref, n_ref


def test_chain_table_writer_i_p_b_in_one_launch(hip_lib):
    """Three chains on three clips, coded I, P, B (coding order of I B P); then ONE x264hip_cavlc_write_chains whose entries are chain 0's
    I slice, chain 1's P slice and chain 2's B slice, each from its own state and at its own QP: every chain's bytes are the reference's for
    that frame.  The I and the P state through x264hip_cavlc_write_frame give the same bytes for those chains."""
    w, h, n, B = 96, 80, 3, 3
    kw = dict(qp=27, me_method=rs.ME_HEX, subme=5, n_refs=2, inter=0x113, intra=0x3, transform8x8=1, cabac=0, deblock=1)
    ekw = dict(bframes=2, weightb=1, direct_pred=rs.DIRECT_SPATIAL)
    clips = [rs.clip(w, h, n, t0) for t0 in (0, 17, 41)]
    want = [rs.run_reference2(rs.make_params(w, h, n, **kw), rs.make_ext(write=1, **ekw), *cl) for cl in clips]
    lib = hip_lib
    enc = sl.ChainEncoder(lib, w, h, cqm_init(lib), batch=B, write=1, **kw, **ekw)
    assert enc.cavlc and enc.raster and not enc.rd_opt["write"]
    n_mb = enc.ctx.dims.mb_w * enc.ctx.dims.mb_h
    cap = enc.payload_cap
    bufs = [dict(payload=DeviceArray(lib, (B, cap), np.uint8), payload_len=DeviceArray(lib, (B,), np.int32), mb_bits=DeviceArray(lib, (B, n_mb), np.int32)) for _ in range(3)]
    tb = lib.x264hip_chain_cavlc_bytes()
    tab_host, tab_dev = lib.x264hip_host_alloc(tb * B), DeviceArray(lib, (tb * B,), np.uint8)
    try:
        frames = []                                    # per coded frame: (slice type, qp, state, list-0 size)
        order = sl.coding_order(n, 0, 2)
        assert [t for _, t in order] == [sl.SLICE_I, sl.SLICE_P, sl.SLICE_B]
        for disp, stype in order:
            for b, (y, u, v) in enumerate(clips):
                enc.upload(y[disp], u[disp], v[disp], b=b)
            st, qp, state = enc.encode_frame(stype=stype, disp=disp)
            enc.status()
            frames.append((st, qp, state, 0 if st == sl.SLICE_I else 1))
            enc.finish_frame()
        assert len({id(f[2]) for f in frames}) == 3 and len({f[1] for f in frames}) == 3      # three resident states, three QPs

        def params(k, rb):
            st, qp, _, n_ref0 = frames[k]
            return sl.CavlcParams(slice_type=st, n_ref0=n_ref0, analyse_inter=kw["inter"], transform8x8=1, cqm_custom=0, payload=rb["payload"].ptr,
                                  payload_cap=cap, payload_len=rb["payload_len"].ptr, mb_bits=rb["mb_bits"].ptr, slice_qp=qp)

        ps = [params(k, bufs[0]) for k in range(3)]
        entries = (sl.ChainCavlc * 3)(*[sl.ChainCavlc(k, C.addressof(frames[k][2].st), C.addressof(ps[k])) for k in range(3)])
        enc.ctx.check(lib.x264hip_cavlc_write_chains(enc.ctx.h, entries, 3, tab_host, tab_dev.p), "cavlc_write_chains")
        single = [params(k, bufs[1 + k]) for k in range(2)]                 # the I and the P state, every chain, by the lock-step entry point
        for k in range(2):
            enc.ctx.check(lib.x264hip_cavlc_write_frame(enc.ctx.h, C.byref(frames[k][2].st), C.byref(single[k])), "cavlc_write_frame")
        enc.ctx.sync()
        enc.status()
        ln, raw, bits = bufs[0]["payload_len"].get(), bufs[0]["payload"].get(), bufs[0]["mb_bits"].get()
        for k in range(3):
            ref = bytes(want[k]["payload"][k, :want[k]["payload_len"][k]])
            got = bytes(raw[k, sl.PAYLOAD_LEAD:sl.PAYLOAD_LEAD + ln[k]])
            assert got == ref, "chain %d (%s slice at QP %d): %d bytes, the reference %d" % (k, "PBI"[frames[k][0]], frames[k][1], len(got), len(ref))
            assert np.array_equal(bits[k], want[k]["mb_bits"][k]), "chain %d: mb_bits" % k
            if k < 2:
                l1, r1 = bufs[1 + k]["payload_len"].get(), bufs[1 + k]["payload"].get()
                assert bytes(r1[k, sl.PAYLOAD_LEAD:sl.PAYLOAD_LEAD + l1[k]]) == got, "chain %d: x264hip_cavlc_write_frame writes other bytes" % k
    finally:
        enc.ctx.sync()
        tab_dev.free()
        lib.x264hip_host_free(tab_host)
        for rb in bufs:
            for d in rb.values():
                d.free()
        enc.close()


def _b_slice_encoder(hip_lib, **over):
    """An encoder that has coded I and P and holds the B picture between them: returns (enc, clip)."""
    w, h = 96, 80
    kw = dict(qp=27, me_method=rs.ME_HEX, subme=5, n_refs=1, inter=0x113, intra=0x3, transform8x8=1, cabac=0, deblock=1, bframes=1, write=1)
    kw.update(over)
    y, u, v = rs.clip(w, h, 3)
    enc = sl.ChainEncoder(hip_lib, w, h, cqm_init(hip_lib), batch=2, **kw)
    for disp, stype in ((0, sl.SLICE_I), (2, sl.SLICE_P)):
        for b in range(2):
            enc.upload(y[disp], u[disp], v[disp], b=b)
        enc.encode_frame(stype=stype, disp=disp)
        enc.status()
        enc.finish_frame()
    for b in range(2):
        enc.upload(y[1], u[1], v[1], b=b)
    return enc


def test_cavlc_b_slice_refusals(hip_lib):
    """Error strings, not approximations: subme 6 with cabac = 0 in a B slice; a CAVLC B slice into a state without level arrays."""
    enc = _b_slice_encoder(hip_lib)
    try:
        enc.opt["subme"] = 6                           # (the encoder itself would have chosen the CABAC-priced RD path; the sweep is asked directly)
        with pytest.raises(RuntimeError, match="CABAC"):
            enc.encode_frame(stype=sl.SLICE_B, disp=1)
    finally:
        enc.close()
    enc = _b_slice_encoder(hip_lib)
    bare = sl.DeviceState(enc.ctx, levels=False)
    try:
        used = [r[0] for r in enc.refs]
        pic_i = next(i for i, p in enumerate(enc.pool) if not any(p is q for q in used))
        full, enc.states[pic_i] = enc.states[pic_i], bare
        with pytest.raises(RuntimeError, match="level arrays"):
            enc.encode_frame(stype=sl.SLICE_B, disp=1)
        enc.states[pic_i] = full
    finally:
        bare.free()
        enc.close()


def test_chain_table_mixing_cabac_and_cavlc_is_refused(hip_lib):
    """x264hip_slice_sweep_chains: one entry with the CABAC coder in the loop, one CAVLC entry without a writer -> an error string."""
    w, h = 96, 80
    cq = cqm_init(hip_lib)
    common = dict(qp=27, me_method=rs.ME_HEX, subme=5, n_refs=1, inter=0x113, intra=0x3, transform8x8=1, deblock=1, write=1, raster=True)
    e_cabac = sl.ChainEncoder(hip_lib, w, h, cq, batch=2, cabac=1, **common)
    e_cavlc = sl.ChainEncoder(hip_lib, w, h, cq, batch=2, cabac=0, **common)
    lib, c = hip_lib, e_cabac.ctx
    tb = lib.x264hip_chain_sweep_bytes()
    tab_host, tab_dev = lib.x264hip_host_alloc(tb * 2), DeviceArray(lib, (tb * 2,), np.uint8)
    try:
        y, u, v = rs.clip(w, h, 1)
        for b in range(2):
            e_cabac.upload(y[0], u[0], v[0], b=b)
        recon, state = e_cabac.pool[0], e_cabac.states[0]

        def launch(encs):
            entries, keep = (ChainSweep * 2)(), []
            for b, e in enumerate(encs):
                p = e.slice_params(sl.SLICE_I, 24, 0, e.cost_table(24).ptr, None)
                rd = e.slice_rd(dict(e.rd_bufs, payload=e_cabac.rd_bufs["payload"], payload_len=e_cabac.rd_bufs["payload_len"], mb_bits=e_cabac.rd_bufs["mb_bits"],
                                     stale=e_cabac.rd_bufs["stale"]), 24.0, 0, None, e.rd_opt["write"], 0)
                rd.payload_cap = e_cabac.payload_cap
                p.rd = C.addressof(rd)
                keep += [p, rd]
                entries[b] = ChainSweep(chain=b, fenc=C.addressof(e_cabac.fenc), refs=None, n_refs=0, recon=C.addressof(recon), params=C.addressof(p), l0=None,
                                        out=C.addressof(state.st))
            c.check(lib.x264hip_mb_state_clear_progress(c.h, C.byref(state.st)), "mb_state_clear_progress")
            c.check(lib.x264hip_slice_sweep_chains(c.h, entries, 2, tab_host, tab_dev.p), "slice_sweep_chains")
            c.sync()

        with pytest.raises(RuntimeError, match="all-CAVLC or not at all"):
            launch([e_cabac, e_cavlc])
        launch([e_cavlc, e_cavlc])                     # the all-CAVLC table is accepted
        c.check(lib.x264hip_slice_sweep_status(c.h, C.byref(state.st)), "slice_sweep_status")
    finally:
        c.sync()
        tab_dev.free()
        lib.x264hip_host_free(tab_host)
        e_cavlc.close()
        e_cabac.close()
