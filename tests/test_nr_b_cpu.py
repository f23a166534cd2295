"""--nr in B slices and under the post-encode scene cut, what needs no GPU (tests/nr_b_cases.py): the committed fixtures are what the
reference gives today and prove what they are there for, the command line accepts the configurations, the C ABI has the per-chain update."""
import os

import numpy as np
import pytest

import edge_cases as ec
import nr_b_cases as nb
from oracle import refslice as rs
from x264_vs2008_amd import encode as E

FIXTURE_LIMIT = 64 << 10          # the existing fixtures of chains this small stay well below it


@pytest.mark.parametrize("name", nb.ALL)
def test_fixture_shows_what_the_case_is_there_for(name):
    """--nr changes the payload of a B frame (of any frame, in a stream), and the post-encode scene cut cases have a given-up attempt."""
    x = nb.fixture(name)
    assert not nb.condition_problems(name, x), nb.condition_problems(name, x)
    assert os.path.getsize(nb.fixture_path(name)) < FIXTURE_LIMIT
    assert (x["frame_info"][:, 0] == rs.SLICE_B).sum() >= 2
    if name in nb.LOCK:
        frames, bf = nb.LOCK[name]["frames"], nb.LOCK[name]["ext"]["bframes"]
        assert frames >= 7 and x["frame_info"][:, 0].tolist()[:2 + bf] == [rs.SLICE_I, rs.SLICE_P] + [rs.SLICE_B] * bf


def test_case_list_covers_both_strengths_and_both_b_patterns():
    for cfg in nb.CONFIGS:
        got = {(c["kw"]["noise_reduction"], c["ext"]["bframes"]) for n, c in nb.LOCK.items() if n.startswith(cfg + "_nr")}
        assert got == {(60, 1), (400, 2)}, cfg
    kws = [c["kw"] for c in nb.LOCK.values()]
    exts = [c["ext"] for c in nb.LOCK.values()]
    assert {2, 4, 5, 6, 7, 8} <= {k["subme"] for k in kws} and any(not k["cabac"] for k in kws) and any(k.get("mixed_refs") and k["n_refs"] == 3 for k in kws)
    assert any(e.get("trellis") == 1 for e in exts) and any(e.get("psy_rd") and e.get("aq_mode") for e in exts)
    assert any(e.get("weightb") and e["direct_pred"] == rs.DIRECT_TEMPORAL for e in exts)
    assert sorted(c["size"] for c in nb.SMALL.values()) == sorted(2 * nb.SMALL_SIZES)


@pytest.mark.skipif(not ec.have_reference(), reason="oracle/_ref/libx264ref.so not built (needs the reference's sources)")
@pytest.mark.parametrize("name", nb.ALL)
def test_fixture_regenerates_to_the_same_bytes(name):
    a, a0 = nb.reference(name)
    x, gold = nb.expected(name, a, a0), nb.fixture(name)
    assert sorted(x) == sorted(gold)
    for k in x:
        assert x[k].dtype == gold[k].dtype and x[k].shape == gold[k].shape and x[k].tobytes() == gold[k].tobytes(), "%s: %s" % (name, k)


def test_check_built_accepts_nr_with_b_frames_and_the_default_scene_cut(hip_lib_host):
    from x264_vs2008_amd import mux
    o = E.build_parser().parse_args("--nr 100 --crf 23 --bframes 3 -o x in.y4m".split())
    p = mux.encoder_params(hip_lib_host, width=176, height=96, fps_num=25, fps_den=1, **E.param_fields(o))
    assert p.noise_reduction == 100 and p.bframe == 3 and not p.pre_scenecut and p.scenecut_threshold >= 0 and E.needs_lookahead(p)
    E.check_built(p)
    for c in nb.CLI.values():
        E.check_built(nb.cli_params(c, hip_lib_host))


def test_abi_declares_the_per_chain_update():
    from x264_vs2008_amd.abi import PROTOTYPES
    assert PROTOTYPES["x264hip_noise_reduction_update_chains"] == "i:ppipi" and PROTOTYPES["x264hip_noise_reduction_update"] == "i:ppi"


def test_stream_encoder_source_has_no_nr_refusal_left():
    """The update moved from the launch to the step: the shared launch code no longer calls the all-chains update."""
    import inspect
    from x264_vs2008_amd import stream
    assert "x264hip_noise_reduction_update(" not in inspect.getsource(stream.StreamEncoder._launch)
    assert "x264hip_noise_reduction_update_chains" in inspect.getsource(stream.StreamEncoder._nr_update)
