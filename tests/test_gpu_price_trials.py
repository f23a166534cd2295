"""GPU: the RD trials' bit count (csrc/cabac_price.h: block summaries balloted by the wave, lane 0 walking them) in the lock-step raster kernels
(I / P, B with spatial and with temporal direct prediction) and in the chain table's I / P and extended B kernels, on the smallest pictures where
it can go wrong: one, two and six macroblocks (tests/edge_cases.py: lane-to-coefficient mapping, contexts without neighbours) and one noisy
64x48 clip, as I P B B P chains of the medium options (3 references, subme 7, trellis 1, psy-rd 1.0, 8x8 transform, mixed references, weighted
bi-prediction) at QP 2 (dense blocks, escape levels) and QP 40 (mostly empty blocks).  A wrong count changes a decision: payload bytes, their
length and every macroblock's type, QP, vectors and coded-block pattern are held to the CPU twin (liboracle.so through oracle/refslice.py)."""
import functools

import numpy as np
import pytest

import edge_cases as E
from oracle import refslice as rs
from psy_table_util import ViaTable
from slice_util import run_chain2
from x264_vs2008_amd import slice as sl

pytestmark = pytest.mark.gpu

FRAMES = 5
PICTURES = ["16x16", "32x16", "40x24", "64x48"]
KW = dict(subme=7, **E.MEDB)
EKW = dict(trellis=1, psy_rd=1.0, bframes=2, weightb=1)
ARRAYS = ("mb_type", "qp", "mv", "cbp")


@functools.lru_cache(maxsize=None)
def picture(name):
    w, h = (int(v) for v in name.split("x"))
    if (w, h) != (64, 48):
        return (w, h), E.clip("noise", (w, h), FRAMES)
    # a noise field that moves two pixels right and one down per frame under a little fresh noise: something to predict from, residuals everywhere
    r = np.random.default_rng(6448)
    field = r.integers(0, 256, (h + FRAMES, w + 2 * FRAMES))
    y = np.stack([np.clip(field[FRAMES - 1 - t:FRAMES - 1 - t + h, 2 * (FRAMES - 1 - t):2 * (FRAMES - 1 - t) + w] + r.integers(-6, 7, (h, w)), 0, 255) for t in range(FRAMES)]).astype(np.uint8)
    y = np.ascontiguousarray(y)
    out = (y, np.ascontiguousarray(y[:, ::2, ::2]), np.ascontiguousarray(255 - y[:, 1::2, 1::2]))
    for a in out:
        a.setflags(write=False)
    return (w, h), out


@functools.lru_cache(maxsize=None)
def twin(name, qp, direct):
    (w, h), (y, u, v) = picture(name)
    a = rs.run2(E.twin_lib(), "x264o_encode_chain2", rs.make_params(w, h, FRAMES, qp=qp, **KW), rs.make_ext(direct_pred=direct, **EKW), y, u, v)
    for arr in a.values():
        arr.setflags(write=False)
    return a


def test_the_chain_is_i_p_b_b_p():
    assert [t for _, t in sl.coding_order(FRAMES, 0, 2)] == [sl.SLICE_I, sl.SLICE_P, sl.SLICE_B, sl.SLICE_B, sl.SLICE_P]


@pytest.mark.parametrize("direct", [1, 2], ids=["spatial", "temporal"])
@pytest.mark.parametrize("path", ["raster", "table"])
@pytest.mark.parametrize("qp", [2, 40])
@pytest.mark.parametrize("name", PICTURES)
def test_trial_pricing_decides_like_the_twin(hip_lib, oracle_lib, cqm, name, qp, path, direct):
    size, (y, u, v) = picture(name)
    want = twin(name, qp, direct)
    batch = 2 if path == "table" else 1
    lib = ViaTable(hip_lib, batch) if path == "table" else hip_lib
    try:
        out = run_chain2(lib, cqm, size, FRAMES, y, u, v, dict(KW, qp=qp), dict(EKW, direct_pred=direct), batch=batch)
    finally:
        if path == "table":
            lib.free()
    if path == "table":
        assert lib.launches == FRAMES
    for f in range(FRAMES):
        for b in range(batch):
            what = "%s QP %d %s (%s direct) frame %d chain %d" % (name, qp, path, "spatial" if direct == 1 else "temporal", f, b)
            for k in ARRAYS:
                got, exp = out[f][k][b], want[k][f]
                assert np.array_equal(got.reshape(exp.shape), exp), "%s: %s differs first at %s" % (what, k, np.argwhere(got.reshape(exp.shape) != exp)[:3].tolist())
            n = int(want["payload_len"][f])
            assert len(out[f]["payload"][b]) == n, "%s: payload_len %d, the twin %d" % (what, len(out[f]["payload"][b]), n)
            assert out[f]["payload"][b] == bytes(want["payload"][f, :n]), "%s: payload bytes differ" % what
