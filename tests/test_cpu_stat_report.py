"""CPU: x264hip_stat_* -- x264_encoder_frame_end's sums and x264_encoder_close's report in the library's host C -- against text built with the reference's
format strings from numbers accumulated in the reference's types (tests/quality_cases.py: RefText), fed with what the REFERENCE measured and counted on its own
pictures and state arrays (tests/golden/quality_chains.npz).  R/encoder/encoder.c needs the configure-generated config.h and is not buildable, so the
reference's own log cannot be produced: the numbers are pinned against its functions and arrays, the text against its format strings."""
import os

import numpy as np
import pytest

import quality_cases as qc
from paths import REF_SO
from x264_vs2008_amd import mux
from x264_vs2008_amd.quality import REPORT_DTYPE, Stat

# the stream-level parameters each case's chain implies (oracle/gen_golden_slice.py: CASES2; MED / MEDB: two references, 8x8 transform)
CONFIG = {"b_medium": dict(bframe=3, frame_reference=2, transform_8x8=1), "rd7_lowqp": dict(bframe=0, frame_reference=2, transform_8x8=1),
          "w_medium_ip": dict(bframe=0, frame_reference=2, transform_8x8=1)}


def feed(lib, name, psnr=1, ssim=1, frames=None, edit=None, **over):
    size = qc.case_config(name)[0]
    cfg = dict(CONFIG[name], **over)
    p = mux.encoder_params(lib, width=size[0], height=size[1], rc_method=mux.RC_CQP, qp_constant=26, **cfg)
    stat = Stat(lib, p, psnr, ssim)
    ref = qc.RefText(size[0], size[1], p.fps_num, p.fps_den, bframe=p.bframe, transform_8x8=p.transform_8x8, direct_auto=int(p.direct_mv_pred == 3), psnr=psnr, ssim=ssim)
    last_anchor = None
    try:
        for f, e in enumerate(qc.load_fixture(name)[:frames]):
            if edit:
                e = edit(f, e)
            size_bytes = e["payload_len"] + 5              # a stated frame size (oracle/ref_slice.c:257 reports payloads the same way)
            idc = 0 if e["stype"] == qc.SLICE_B else 3 if f == 0 else 2
            since = 0 if last_anchor is None else e["disp"] - last_anchor - 1
            spatial = f % 2
            got = stat.frame_end(qc.record_of(e), e["stype"], size_bytes, nal_ref_idc=idc, poc=e["poc"], frames_since_ref=since, direct_spatial=spatial)
            want = ref.frame_end(e, size_bytes, idc, since, spatial)
            assert got == want, "frame %d" % f
            if e["stype"] != qc.SLICE_B:
                last_anchor = e["disp"]
        assert stat.frames == ref.i_frame
        got, want = stat.summary(), ref.summary()
        assert got == want
        assert stat.summary() == got                       # printing changes nothing
        return got
    finally:
        stat.close()


@pytest.mark.parametrize("name", qc.CASES)
def test_frame_lines_and_closing_report_equal_the_reference_format(hip_lib_host, name):
    text = feed(hip_lib_host, name)
    lines = text.splitlines()
    assert all(l.startswith("x264 [info]: ") for l in lines)
    assert lines[0].startswith("x264 [info]: slice I:1 ") and "PSNR Mean Y:" in lines[0] and lines[-1].startswith("x264 [info]: PSNR Mean Y:") and " kb/s:" in lines[-1]
    assert lines[-2].startswith("x264 [info]: SSIM Mean Y:0.9")
    assert any(l.startswith("x264 [info]: 8x8 transform  intra:") for l in lines)
    beyond_ref0 = any(e["stype"] == qc.SLICE_P and e["mb_count_ref"][0, 1:].any() for e in qc.load_fixture(name))
    assert any(l.startswith("x264 [info]: ref P L0 ") for l in lines) == beyond_ref0          # (i_max == 0: the line is left out)
    assert ("consecutive B-frames:" in text) == (name == "b_medium") == ("mb B  I16..4" in text)
    assert "direct mvs" not in text


def test_anchor_numbers_are_in_the_fixture():
    """The fixture's generator against the figures of a separate CPU run of the reference's functions (frames 0 and 1 of w_medium_ip)."""
    ex = qc.load_fixture("w_medium_ip")
    for f in (0, 1):
        ssd, mean = qc.ANCHORS[("w_medium_ip", f)]
        assert ex[f]["ssd"].tolist() == ssd and abs(ex[f]["f_ssim"] / (((208 - 6) >> 2) * ((144 - 6) >> 2)) - mean) < 5e-10
        assert ex[f]["f_ssim"] == sum(float(x) for x in ex[f]["parts"])       # the calls' floats, added in call order into a double
    with np.load(qc.FIXTURE) as z:
        n_diff, n_all = z["order_visible"].tolist()
    assert n_all == 114 and n_diff >= 112                  # one whole-frame call almost never gives the chunked sum's bits: the comparison is on bits


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (the reference's sources are absent): the fixture stands")
def test_fixture_is_what_the_reference_functions_give_now():
    m = qc.Measure("ref")
    for name in qc.CASES:
        for f, (a, b) in enumerate(zip(qc.expected_for_case(m, name), qc.load_fixture(name))):
            qc.same_record(qc.record_of(a), qc.record_of(b), "%s frame %d" % (name, f))
            assert a["parts"].tobytes() == b["parts"].tobytes()


def test_zero_error_is_100_db(hip_lib_host):
    def edit(f, e):
        return dict(e, ssd=np.zeros(3, np.int64)) if f == 0 else e
    text = feed(hip_lib_host, "w_medium_ip", edit=edit, frames=1, transform_8x8=0)
    assert "PSNR Mean Y:100.00 U:100.00 V:100.00 Avg:100.00 Global:100.00" in text and "PSNR Mean Y:100.000 U:100.000 V:100.000 Avg:100.000 Global:100.000" in text


def test_psnr_off_selects_the_short_lines(hip_lib_host):
    text = feed(hip_lib_host, "b_medium", psnr=0)
    assert "PSNR" not in text and text.splitlines()[-1].startswith("x264 [info]: kb/s:") and "SSIM Mean Y:" in text
    assert all(l.rstrip()[-1].isdigit() for l in text.splitlines() if l.startswith("x264 [info]: slice "))
    text = feed(hip_lib_host, "b_medium", psnr=0, ssim=0)
    assert "SSIM" not in text


def test_conditions_of_the_closing_report(hip_lib_host):
    assert "8x8 transform" not in feed(hip_lib_host, "w_medium_ip", transform_8x8=0)

    def one_ref(f, e):
        return dict(e, mb_count_ref=np.zeros((2, 32), np.int32))          # i_frame_reference == 1: x264_slice_write counts no references
    assert "\nx264 [info]: ref " not in feed(hip_lib_host, "b_medium", edit=one_ref)
    text = feed(hip_lib_host, "b_medium", direct_mv_pred=3)
    assert "x264 [info]: direct mvs  spatial:" in text
    assert "consecutive B-frames" not in feed(hip_lib_host, "b_medium", frames=1, transform_8x8=0)          # no P slice yet


def test_lossless_turns_both_measurements_off(hip_lib_host):
    p = mux.encoder_params(hip_lib_host, width=96, height=80, rc_method=mux.RC_CQP, qp_constant=0)
    assert p.d_lossless
    stat = Stat(hip_lib_host, p, 1, 1)
    try:
        line = stat.frame_end(np.zeros((), REPORT_DTYPE), qc.SLICE_I, 100, nal_ref_idc=3)
        assert "PSNR" not in line and "SSIM" not in line and "PSNR" not in stat.summary() and "SSIM" not in stat.summary()
    finally:
        stat.close()
