"""GPU: the P 8x8 analysis searches a block against all its references at once (me_exact.h: me_search_refs8, four references per
pass), and must decide exactly what the serial loop of x264_mb_analyse_inter_p8x8_mixed_ref decides.  Chains of the raster-order
variant with 2, 3, 5 and 6 references (one pass, two passes), mixed references on and off, hex and the methods that keep the serial
search (dia, umh), subme 6-9, and small or odd frames whose vectors clip at the picture borders and at a short --mv-range -- every
decision, level, pixel and payload byte against the reference's own loop where oracle/_ref is built, and its CPU twin otherwise."""
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import refslice as rs
from oracle.gen_golden_slice import case_inputs, masked
from slice_util import check_frame, run_chain2

pytestmark = pytest.mark.gpu

P = dict(inter=0x13, intra=0x3, transform8x8=1, cabac=1, deblock=1)
CASES = [
    # name, size, frames, clip, analysis options, extension options
    ("hex_ref3_mixed_rd7", (208, 144), 6, "moving", dict(qp=26, subme=7, me_method=rs.ME_HEX, n_refs=3, mixed_refs=1, **P), dict(trellis=1, psy_rd=1.0, aq_mode=1)),
    ("hex_ref2_mixed_rd6", (112, 80), 5, "static", dict(qp=30, subme=6, me_method=rs.ME_HEX, n_refs=2, mixed_refs=1, **P), dict(trellis=1)),
    ("hex_ref5_mixed_rd7_odd", (72, 56), 8, "moving", dict(qp=24, subme=7, me_method=rs.ME_HEX, n_refs=5, mixed_refs=1, **P), dict(psy_rd=1.0)),
    ("hex_ref6_mixed_rd8", (112, 80), 8, "moving", dict(qp=28, subme=8, me_method=rs.ME_HEX, n_refs=6, mixed_refs=1, **P), dict(trellis=1, psy_rd=1.0)),
    ("hex_ref6_mixed_rd9_range", (88, 72), 8, "static", dict(qp=22, subme=9, me_method=rs.ME_HEX, me_range=8, n_refs=6, mixed_refs=1, mv_range=64, **P),
     dict(trellis=2)),
    ("hex_ref3_nomixed_rd7", (208, 144), 5, "moving", dict(qp=26, subme=7, me_method=rs.ME_HEX, n_refs=3, mixed_refs=0, **P), dict(trellis=1, psy_rd=1.0)),
    ("hex_ref3_mixed_rd7_chroma_me_off", (80, 72), 5, "moving", dict(qp=30, subme=7, me_method=rs.ME_HEX, n_refs=3, mixed_refs=1, chroma_me=0, **P),
     dict(trellis=1)),
    ("umh_ref3_mixed_rd7", (112, 80), 5, "moving", dict(qp=28, subme=7, me_method=rs.ME_UMH, n_refs=3, mixed_refs=1, **P), dict(trellis=1, psy_rd=1.0)),
    ("dia_ref5_mixed_rd6", (112, 80), 7, "static", dict(qp=32, subme=6, me_method=rs.ME_DIA, n_refs=5, mixed_refs=1, **P), dict()),
]


def want_chain(size, frames, y, u, v, kw, ekw):
    """The reference's loop (refslice_encode_chain2) where it is built, the CPU twin (x264o_encode_chain2) otherwise."""
    p, e = rs.make_params(size[0], size[1], frames, **kw), rs.make_ext(**ekw)
    if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libx264ref.so")):
        return rs.run_reference2(p, e, y, u, v)
    import ctypes
    return rs.run2(ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so")), "x264o_encode_chain2", p, e, y, u, v)


@pytest.mark.parametrize("name,size,frames,kind,kw,ekw", CASES, ids=[c[0] for c in CASES])
def test_p8x8_reference_search_matches_serial_loop(hip_lib, cqm, name, size, frames, kind, kw, ekw):
    y, u, v = case_inputs(size, frames, kind)
    gold = masked(want_chain(size, frames, y, u, v, kw, ekw))
    out = run_chain2(hip_lib, cqm, size, frames, y, u, v, kw, ekw)
    for f in range(frames):
        check_frame(out[f], gold, f, kw["n_refs"])
        n = int(gold["payload_len"][f])
        assert out[f]["payload"][0] == bytes(gold["payload"][f, :n]), "frame %d: payload differs" % f
