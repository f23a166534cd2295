"""The CAVLC writer (x264hip_cavlc_write_frame: x264_macroblock_write_cavlc + the skip runs of x264_slice_write as a pass over the state the
wavefront variant leaves) against the REFERENCE's own writer run inside its per-macroblock loop (oracle/ref_slice.c refslice_encode_chain2
with cabac = 0): the slice_data() bytes of every frame of I / P chains -- BASELINE config 0's shape (352x288, dia, subme 0, no partitions)
and richer ones (all P partitions incl. sub-8x8, several references, 8x8 transform with its coefficient interleave, intra-heavy low QP).

  * golden: tests/golden/cavlc_*.npz made by oracle/gen_golden_cavlc.py from the reference;
  * live: the same configurations on other clips where oracle/_ref/libx264ref.so is built;
  * hand-built worst-case macroblocks against the host-compiled writer, a payload slot too small, and what the entry points refuse."""
import ctypes as C
import os

import numpy as np
import pytest

import cavlc_synth as S
from cavlc_host_util import MB_BYTES_MAX, STATE_ARRAYS, write_state
from cavlc_util import CONFIGS, encode, reference
from oracle import refslice as rs
from paths import REF_SO, ROOT
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd.frame import DeviceArray, FrameCtx, cqm_init

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_cavlc_payload_equals_reference_fixture(hip_lib, name):
    c = CONFIGS[name]
    gold = np.load(os.path.join(ROOT, "tests", "golden", "cavlc_%s.npz" % name))
    got = encode(hip_lib, c, rs.clip(c["w"], c["h"], c["n"], 0))
    for f in range(c["n"]):
        want = bytes(gold["payload"][f, :gold["payload_len"][f]])
        assert got[f] == want, "%s frame %d: CAVLC payload differs (%d vs %d bytes)" % (name, f, len(got[f]), len(want))


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs /root/reference)")
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_cavlc_payload_equals_reference_live(hip_lib, name):
    c = CONFIGS[name]
    clip, want, _ = reference(c, t0=37)
    got = encode(hip_lib, c, clip)
    for f in range(c["n"]):
        assert got[f] == want[f], "%s frame %d: CAVLC payload differs (%d vs %d bytes)" % (name, f, len(got[f]), len(want[f]))


def test_cavlc_batch_of_chains(hip_lib):
    """Several chains per launch: every chain's payload is the single-chain one."""
    c = CONFIGS["p_no_sub8x8_umh"]
    clips = [rs.clip(c["w"], c["h"], c["n"], t0) for t0 in (0, 11, 23)]
    single = [encode(hip_lib, c, cl) for cl in clips]
    enc = sl.ChainEncoder(hip_lib, c["w"], c["h"], cqm_init(hip_lib), batch=3, write=1, **c["kw"])
    try:
        for f in range(c["n"]):
            for b, (y, u, v) in enumerate(clips):
                enc.upload(y[f], u[f], v[f], b=b)
            enc.encode_frame()
            enc.status()
            pay = enc.payloads()
            for b in range(3):
                assert pay[b] == single[b][f], "chain %d frame %d" % (b, f)
            enc.finish_frame()
    finally:
        enc.close()


def test_full_slot_refusals_and_worst_case_macroblocks(hip_lib):
    """Hand-built states of worst-case macroblocks (tests/cavlc_synth.py: what no quantiser produces and the C ABI accepts) through both entry
    points.  With room, the kernel's bytes are the host-compiled writer's (read back and measured by tests/test_cavlc_host.py).  With a
    payload_cap under which the fourth macroblock begins 1040 bytes before the slot's end -- I and P slices of x264hip_cavlc_write_frame,
    a chain of x264hip_cavlc_write_chains --: the call succeeds, the status call reports the abort, the length is 0 and the next chain's slot,
    filled with a pattern, stays as it was (both slots lie in one allocation).  And what the entry points refuse before any launch."""
    lib = hip_lib
    ctx = FrameCtx(lib, 16 * S.MB_W, 16 * S.MB_H)
    state, bare = sl.DeviceState(ctx), sl.DeviceState(ctx, levels=False)
    roomy = sl.PAYLOAD_LEAD + (S.N + 1) * MB_BYTES_MAX
    plen = DeviceArray(lib, (2,), np.int32)
    tab_host, tab_dev = lib.x264hip_host_alloc(lib.x264hip_chain_cavlc_bytes()), DeviceArray(lib, (lib.x264hip_chain_cavlc_bytes(),), np.uint8)
    bufs = [plen, tab_dev]
    assert state.st.mv1 and state.st.ref1

    def params(kind, buf, cap, **k):
        p = S.params(kind, 1)
        return sl.CavlcParams(**dict(dict(slice_type=p["slice_type"], n_ref0=p["n_ref0"], analyse_inter=p["inter"], transform8x8=p["transform8x8"], cqm_custom=0,
                                          payload=buf.ptr, payload_cap=cap, payload_len=plen.ptr, mb_bits=None, slice_qp=p["slice_qp"]), **k))

    def launch(entry, st, cp):
        if entry == "frame":
            return lib.x264hip_cavlc_write_frame(ctx.h, C.byref(st), C.byref(cp))
        e = (sl.ChainCavlc * 1)(sl.ChainCavlc(chain=0, state=C.addressof(st), params=C.addressof(cp)))
        return lib.x264hip_cavlc_write_chains(ctx.h, e, 1, tab_host, tab_dev.p)

    try:
        for entry, kind in (("frame", "i16"), ("frame", "p8"), ("chains", "i16")):
            what = "%s, %s" % (entry, kind)
            host = S.state(kind, "min")
            for k in STATE_ARRAYS:
                a = np.ascontiguousarray(host[k])
                assert lib.x264hip_memcpy_h2d(getattr(state.st, k), a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
            rc, want, want_len, bits = write_state(host, S.MB_W, S.MB_H, cap=roomy, **S.params(kind, 1))
            assert rc == 0
            for cap in (roomy, S.full_slot_cap(bits)):
                guard = DeviceArray(lib, (2, cap), np.uint8, np.full((2, cap), 0xA5, np.uint8))
                bufs.append(guard)
                plen.set(np.full(2, -1, np.int32))
                ctx.check(lib.x264hip_mb_state_clear_progress(ctx.h, C.byref(state.st)), "mb_state_clear_progress")
                assert launch(entry, state.st, params(kind, guard, cap)) == 0, "%s: %s" % (what, lib.x264hip_last_error().decode())
                status = lib.x264hip_slice_sweep_status(ctx.h, C.byref(state.st))
                raw, n = guard.get(), int(plen.get()[0])
                assert (raw[1] == 0xA5).all(), "%s, payload_cap %d: the writer wrote behind its slot" % (what, cap)
                if cap == roomy:
                    assert status == 0, "%s: %s" % (what, lib.x264hip_last_error().decode())
                    assert n == want_len and bytes(raw[0, sl.PAYLOAD_LEAD:sl.PAYLOAD_LEAD + n]) == bytes(want[0, sl.PAYLOAD_LEAD:sl.PAYLOAD_LEAD + n]), \
                        "%s: the kernel's slice (%d bytes) differs from the host writer's (%d)" % (what, n, want_len)
                else:
                    assert status == -1 and "out of payload space" in lib.x264hip_last_error().decode(), what
                    assert n == 0 and (raw[0, sl.PAYLOAD_LEAD:] != 0xA5).any(), what
        # refused before any launch
        ctx.check(lib.x264hip_mb_state_clear_progress(ctx.h, C.byref(state.st)), "mb_state_clear_progress")
        guard = bufs[-1]
        no_l1 = sl.MbState.from_buffer_copy(state.st)
        no_l1.mv1 = None
        for entry in ("frame", "chains"):
            for st, kind, k, word in ((state.st, "i16", dict(payload=None), "payload buffers"), (state.st, "i16", dict(payload_len=None), "payload buffers"),
                                      (bare.st, "i16", {}, "coefficient levels"), (no_l1, "b8", {}, "list-1 arrays"), (state.st, "i16", dict(slice_type=3), "slice type"),
                                      (state.st, "i16", dict(payload_cap=4095 if entry == "frame" else sl.PAYLOAD_LEAD + MB_BYTES_MAX - 1),
                                       "payload_cap" if entry == "frame" else "smaller than one macroblock")):
                rc = launch(entry, st, params(kind, guard, roomy, **k))
                assert rc == -1 and word in lib.x264hip_last_error().decode(), (entry, k, lib.x264hip_last_error().decode())
        cp = params("i16", guard, roomy)
        e = (sl.ChainCavlc * 1)(sl.ChainCavlc(chain=1, state=C.addressof(state.st), params=C.addressof(cp)))
        assert lib.x264hip_cavlc_write_chains(ctx.h, e, 1, tab_host, tab_dev.p) == -1 and "chain 1" in lib.x264hip_last_error().decode()
        assert lib.x264hip_cavlc_write_chains(ctx.h, e, 1, None, tab_dev.p) == -1 and "missing" in lib.x264hip_last_error().decode()
        wide = FrameCtx(lib, 16 * 513, 16)                 # one row of 513 macroblocks: beyond the writer's row of coefficient totals
        wide_state = sl.DeviceState(wide)
        try:
            assert lib.x264hip_cavlc_write_frame(wide.h, C.byref(wide_state.st), C.byref(cp)) == -1
            assert "macroblocks per row" in lib.x264hip_last_error().decode()
        finally:
            wide_state.free()
            wide.close()
        assert lib.x264hip_slice_sweep_status(ctx.h, C.byref(state.st)) == 0 and (guard.get()[1] == 0xA5).all()
    finally:
        ctx.sync()
        for d in bufs:
            d.free()
        lib.x264hip_host_free(tab_host)
        state.free()
        bare.free()
        ctx.close()
