"""`--no-cabac` through the frame queue: the StreamEncoder with cabac = 0 (chain-table raster kernels without their writer, then
x264hip_cavlc_write_chains) and the command line in front of it, against the REFERENCE's whole encoder with b_cabac = 0
(oracle/ref_slice.c refslice_encode_stream): the order frames are coded in, their types, QPs and payload bytes; for the command line the
Annex B file against mux.AnnexB around the reference's payloads.  Equality throughout."""
import os

import pytest

import mux_cases as tm
from cavlc_b_util import STREAMS, run_cavlc_stream, stream_reference
from oracle import refslice as rs
from paths import REF_SO
from stream_util import check
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import mux

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref/libx264ref.so not built (needs the reference tree)")]


@pytest.mark.parametrize("pipeline", [False, True])
def test_cavlc_crf_stream_with_post_encode_scenecut(hip_lib, pipeline):
    """--no-cabac --crf 23 --bframes 0, the default scene cut, a scene change in the clip: the P picture at the change is given up and coded
    again as an intra picture inside the step (the verdict reads the state, not the payload)."""
    c = STREAMS["crf_postsc"]
    a = stream_reference(c)
    assert int(a["stat"][:c["frames"], 3].sum()) > 0, "the reference gives no attempt up: the clip does not test the second attempt"
    assert (a["frame_info"][1:c["frames"], 0] == rs.SLICE_I).any(), "the reference codes no intra picture at the scene change"
    got, _, given_up = run_cavlc_stream(hip_lib, c, pipeline)
    check(got, a, c, "crf_postsc")
    assert given_up == int(a["stat"][:c["frames"], 3].sum())


def test_cavlc_crf_stream_with_adaptive_b_frames_and_direct_auto(hip_lib):
    """--no-cabac --crf 23 --bframes 3 --b-adapt 1 --direct auto: I, P and B chains' slices from one chain-table writer launch per step."""
    c = STREAMS["crf_badapt1_direct_auto"]
    a = stream_reference(c)
    isb = a["frame_info"][:c["frames"], 0] == rs.SLICE_B
    assert isb.sum() >= 3, "the reference places %d B frames" % isb.sum()
    got, spatial, _ = run_cavlc_stream(hip_lib, c)
    check(got, a, c, "crf_badapt1_direct_auto")
    for f in range(c["frames"]):
        if isb[f]:
            assert spatial[f] == int(a["frame_info2"][f][3]), "coded frame %d: direct mode" % f


CLI = {
    "crf": "--no-cabac --crf 23 --subme 5 --me hex --ref 2 --bframes 0 --partitions p8x8,b8x8,i8x8,i4x4 --8x8dct",
    "bframes2": "--no-cabac --crf 23 --subme 5 --me hex --ref 2 --bframes 2 --b-adapt 1 --weightb --partitions p8x8,b8x8,i8x8,i4x4 --8x8dct",
}


@pytest.mark.parametrize("name", sorted(CLI))
def test_cavlc_command_line_equals_reference_stream(hip_lib, tmp_path, name):
    """python -m x264_vs2008_amd.encode --no-cabac --crf 23 ... on a raw clip: the .264 is the Annex B stream around the reference's payloads."""
    w, h, n = 96, 80, 10
    src, out = tmp_path / ("clip_%dx%d.yuv" % (w, h)), tmp_path / "out.264"
    tm.write_clip(str(src), w, h, n)
    args = CLI[name].split()
    assert E.main(args + ["-o", str(out), str(src)]) == 0
    o = E.build_parser().parse_args(args + ["-o", "x.264", str(src)])
    p = mux.encoder_params(hip_lib, width=w, height=h, **E.param_fields(o))
    assert not p.cabac and not p.trellis
    a = tm.reference_med(p, w, h, n)
    want = tm.mux_reference_stream(hip_lib, p, a, n)
    got = out.read_bytes()
    assert got == want, "%s: %d bytes, the reference's stream %d (first difference at %d)" % (
        name, len(got), len(want), next((i for i, (x, z) in enumerate(zip(got, want)) if x != z), min(len(got), len(want))))
    if name == "bframes2":
        assert (a["frame_info"][:n, 0] == rs.SLICE_B).any(), "the reference places no B frame"
