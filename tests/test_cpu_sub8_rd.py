"""Sub-8x8 P partitions under the RD levels, without a GPU: the CPU twin equals every new fixture of tests/sub8_rd_cases.py (decisions, levels,
reconstruction, payload bytes), the fixtures show what they are there for (the condition is checked on the reference's arrays), the ABI record
carries mb_carry, and the encoders refuse what is not built before they allocate anything."""
import ctypes as C

import numpy as np
import pytest

import sub8_rd_cases as SC
from oracle import refslice as rs
from x264_vs2008_amd import abi


@pytest.mark.parametrize("name", sorted(n for n, c in SC.CHAINS.items() if not c["ext"].get("psy_trellis")))
def test_twin_equals_the_fixture(oracle_lib, name):
    """(Every chain case but the psy-trellis ones: the twin has no psy-trellis, x264o_encode_chain2 returns -3 for it; those pin the GPU alone.)"""
    want = SC.fixture(name)
    got = SC.to_fixture(SC.twin(oracle_lib, name))
    n = want["payload_len"]
    assert np.array_equal(got["payload_len"], n), "payload_len %s, the reference %s" % (got["payload_len"].tolist(), n.tolist())
    for f in range(len(n)):
        assert np.array_equal(got["payload"][f, :n[f]], want["payload"][f, :n[f]]), "payload of frame %d differs" % f
    if SC.CHAINS[name].get("pcm"):
        # the twin dumps an I_PCM macroblock's unfiltered reconstruction before its writer copies the source into it (its frame, and with it fin_* and
        # every later frame, has the source): rec_* is compared outside those macroblocks
        mb_w = (SC.CHAINS[name]["size"][0] + 15) // 16
        pcm = (want["mb_type"] == rs.I_PCM).reshape(len(n), -1, mb_w)
        for k, s in (("rec_y", 16), ("rec_u", 8), ("rec_v", 8)):
            m = np.repeat(np.repeat(pcm, s, 1), s, 2)[:, :want[k].shape[1], :want[k].shape[2]]
            got[k], want[k] = np.where(m, 0, got[k]), np.where(m, 0, want[k])
        assert pcm.any()
    for k in want:
        if k != "payload":
            assert np.array_equal(got[k], want[k]), "%s differs first at %s" % (k, np.argwhere(got[k] != want[k])[:3].tolist())


@pytest.mark.parametrize("name", SC.ALL)
def test_fixture_shows_sub_partitions(name):
    x = SC.fixture(name)
    assert not SC.condition_problems(name, x), SC.condition_problems(name, x)
    st = x["frame_info"][:, 0].tolist()
    assert rs.SLICE_I in st and rs.SLICE_P in st and rs.SLICE_B not in st


def test_every_sub_partition_shape_occurs():
    tot = np.zeros(3, int)
    for name in SC.ALL:
        tot += SC.sub_blocks(SC.fixture(name))
    assert (tot > 0).all(), "4x4 / 8x4 / 4x8 blocks over all cases: %s" % tot.tolist()


def test_abi_record_has_the_carry_last():
    f = abi.SliceRd._fields_[-1]
    assert f[0] == "mb_carry" and abi.SliceRd.mb_carry.offset == C.sizeof(abi.SliceRd) - 8


def test_encoders_refuse_what_is_not_built(hip_lib_host, cqm):
    from x264_vs2008_amd import shard
    from x264_vs2008_amd.stream import AsyncStreamEncoder, StreamEncoder
    rd = dict(qp=24, subme=7, me_method=1, n_refs=1, inter=0x33, intra=0x3, transform8x8=1, cabac=1)
    with pytest.raises(ValueError, match="mb_carry"):
        AsyncStreamEncoder(hip_lib_host, 48, 32, cqm, n_frames=4, crf=23.0, **rd)
    with pytest.raises(ValueError, match="bframes"):
        StreamEncoder(hip_lib_host, 48, 32, cqm, crf=23.0, bframes=2, **rd)
    with pytest.raises(ValueError, match="mb_carry"):
        shard.encode_clip(hip_lib_host, cqm, [], 2, **rd)


def test_command_line_refuses_b_frames_with_sub8_rd(hip_lib_host):
    from x264_vs2008_amd import encode as E, mux
    o = E.build_parser().parse_args("--crf 23 --bframes 2 --subme 7 --partitions all -o x in_48x32.yuv".split())
    p = mux.encoder_params(hip_lib_host, width=48, height=32, fps_num=25, fps_den=1, **E.param_fields(o))
    with pytest.raises(ValueError, match="bframes"):
        E.check_built(p)
    o = E.build_parser().parse_args("--crf 23 --bframes 0 --subme 7 --partitions all -o x in_48x32.yuv".split())
    E.check_built(mux.encoder_params(hip_lib_host, width=48, height=32, fps_num=25, fps_den=1, **E.param_fields(o)))
