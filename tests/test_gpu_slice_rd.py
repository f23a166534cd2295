"""GPU: the raster-order variant of the sweep (include/x264hip.h: x264hip_slice_rd) -- the RD levels (subme 6 / 7), trellis,
psy-rd, adaptive quantisation and the CABAC entropy coder inside the macroblock loop -- against chains the REFERENCE's own loop
produced with x264_macroblock_write_cabac in it (oracle/ref_slice.c refslice_encode_chain2, fixtures tests/golden/slice2_*.npz):
every decision, level and pixel as in test_gpu_slice.py (the drivers: tests/slice_util.py), the per-macroblock QP, AND the slice payload bytes."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle.gen_golden_slice import CASES2, case_inputs
from slice_util import check_frame, run_chain2
from x264_vs2008_amd import slice as sl

pytestmark = pytest.mark.gpu


IP_CASES2 = [c for c in CASES2 if not c[5].get("bframes")]        # the kernel codes I and P slices; the B chains pin the twin (round 3: the kernel)


@pytest.mark.parametrize("name,size,frames,kind,kw,ekw", IP_CASES2, ids=[c[0] for c in IP_CASES2])
def test_raster_sweep_matches_reference_loop_and_payload(hip_lib, cqm, name, size, frames, kind, kw, ekw):
    with np.load(os.path.join(GOLDEN, "slice2_%s.npz" % name)) as z:
        gold = {k: z[k] for k in z.files}
    y, u, v = case_inputs(size, frames, kind)
    out = run_chain2(hip_lib, cqm, size, frames, y, u, v, kw, ekw)
    for f in range(frames):
        n = int(gold["payload_len"][f])
        want = bytes(gold["payload"][f, :n])
        # the decisions first (their message says where), then the bytes
        check_frame(out[f], gold, f, kw.get("n_refs", 1))
        assert out[f]["payload"][0] == want, "frame %d: payload differs (%d vs %d bytes)" % (f, len(out[f]["payload"][0]), n)


def test_raster_sweep_batched_chains(hip_lib, cqm):
    """Three chains in one launch (one wavefront each): every element must equal the golden chain, bytes included."""
    name, size, frames, kind, kw, ekw = next(c for c in CASES2 if c[0] == "rd7_aq")
    with np.load(os.path.join(GOLDEN, "slice2_%s.npz" % name)) as z:
        gold = {k: z[k] for k in z.files}
    y, u, v = case_inputs(size, frames, kind)
    out = run_chain2(hip_lib, cqm, size, frames, y, u, v, kw, ekw, batch=3)
    for f in range(frames):
        n = int(gold["payload_len"][f])
        for b in range(3):
            check_frame(out[f], gold, f, kw.get("n_refs", 1), b=b)
            assert out[f]["payload"][b] == bytes(gold["payload"][f, :n])


def test_payload_only_states_and_a_full_payload_buffer(hip_lib, cqm):
    """levels=False (X264HIP_STATE_NO_LEVELS: the states carry no coefficient-level arrays, the payload is the product) gives the
    same bytes; and a payload buffer the slice does not fit stops the sweep with an error instead of writing past it."""
    name, size, frames, kind, kw, ekw = next(c for c in CASES2 if c[0] == "rd7_aq")
    with np.load(os.path.join(GOLDEN, "slice2_%s.npz" % name)) as z:
        gold = {k: z[k] for k in z.files}
    y, u, v = case_inputs(size, frames, kind)
    kw = dict(kw)
    kw.pop("cqm_preset", 0)
    ekw = {k: v_ for k, v_ in ekw.items() if k != "write"}
    enc = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, batch=1, write=1, levels=False, **kw, **ekw)
    try:
        assert not enc.states[0].st.luma and not enc.states[0].st.chroma_ac and enc.states[0].st.mv
        for f in range(frames):
            enc.upload(y[f], u[f], v[f])
            enc.encode_frame()
            enc.status()
            assert enc.payloads()[0] == bytes(gold["payload"][f, :int(gold["payload_len"][f])]), "frame %d" % f
            enc.finish_frame()
    finally:
        enc.close()
    # (at QP 6 the first slice of this clip is far beyond the 2 KB such a buffer leaves before the guard's margin: one macroblock's proven worst case)
    enc = sl.ChainEncoder(hip_lib, size[0], size[1], cqm, batch=1, write=1, payload_cap=8192 + 128 + 2048 + sl.PAYLOAD_LEAD, **dict(kw, qp=6), **ekw)
    try:
        enc.upload(y[0], u[0], v[0])
        enc.encode_frame()
        with pytest.raises(RuntimeError, match="aborted"):
            enc.status()
    finally:
        enc.close()
