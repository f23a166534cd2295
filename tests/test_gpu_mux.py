"""The whole Annex B stream (x264_vs2008_amd/mux.py: version SEI, SPS, PPS, slice headers around the sweep's payloads) against the md5 of
the .264 file the REFERENCE's command line wrote for BASELINE's configurations -- the known-answer values of SURVEY.md 8(c), produced in
the survey from the real `x264 --no-asm --threads 1 <flags>` on the integer synthetic clips of SURVEY.md 8(d) (whose own md5s are checked
here first).  This is the one pin the header writers have: R/encoder/set.c and encoder.c cannot be built here (they need the
configure-generated config.h), so there is no live comparison; an md5 covers every byte -- parameter sets, SEI text, every slice header,
every payload, the emulation prevention."""
import hashlib

import pytest

import mux_cases as M
from mux_cases import clip, med_stream, uf_stream
from x264_vs2008_amd import mux

pytestmark = pytest.mark.gpu

CLIP_MD5, STREAM_MD5 = M.CLIP_MD5, M.STREAM_MD5          # SURVEY.md 8(c) / BASELINE.md 2: md5 of the reference CLI's output, --threads 1


def test_c1_uf_cif30_stream_md5(hip_lib):
    frames, md5 = clip(352, 288, 30)
    assert md5 == CLIP_MD5["cif30"]
    nals = uf_stream(hip_lib, frames)
    stream = b"".join(nals)
    got = hashlib.md5(stream).hexdigest()
    assert got == STREAM_MD5["C1_UF_cif30"], "%d bytes, frames %s, head %s" % (len(stream), [len(n) for n in nals], stream[:160].hex())


@pytest.mark.parametrize("cfg", ["C2_MED_hd24", "C3_MED_umh_uhd8"])
def test_med_stream_md5(hip_lib, cfg):
    """BASELINE configs 2 (the metric's) and 3, as BASELINE.md states them -- no --pre-scenecut: every byte of the product's stream equals the
    reference command line's."""
    import mux_cases as M
    w, h, n, kw = (1920, 1080, 24, M.MED) if cfg == "C2_MED_hd24" else (3840, 2160, 8, dict(M.MED, me_method=2))
    p = mux.encoder_params(hip_lib, width=w, height=h, **kw)
    nals, order = med_stream(hip_lib, p, w, h, n)
    stream = b"".join(nals)
    assert len(nals) == n, order
    assert hashlib.md5(stream).hexdigest() == M.STREAM_MD5[cfg], "%d bytes, coded %s" % (len(stream), order)


def test_c4_slow_stream_md5(hip_lib):
    """BASELINE config 4's flag set as stated (SLOW: --ref 5 --b-adapt 2 --me umh --subme 8 --direct auto, the post-encode scene cut) on hd24:
    the product's stream has the md5 of the reference command line's file.  --direct auto: every B macroblock predicts both direct modes, the
    running skip scores pick each B frame's mode (temporal for the first, spatial later on this clip)."""
    import mux_cases as M
    p = mux.encoder_params(hip_lib, width=1920, height=1080, **M.SLOW)
    nals, order = med_stream(hip_lib, p, 1920, 1080, 24)
    stream = b"".join(nals)
    assert len(nals) == 24, order
    assert hashlib.md5(stream).hexdigest() == M.STREAM_MD5["C4_SLOW_hd24"], "%d bytes, coded %s" % (len(stream), order)
