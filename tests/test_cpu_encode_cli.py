"""The command line front end (x264_vs2008_amd/encode.py) without a GPU: its option parser against the REFERENCE's own x264_param_parse fed the
same options (x264_param2string of both, before validation), and the raw I420 / YUV4MPEG2 readers (R/muxers.c)."""
import os

import numpy as np
import pytest

from mux_cases import ARGS, reference_string
from paths import REF_SO, ROOT
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import mux, synth


@pytest.mark.parametrize("name", sorted(ARGS))
def test_cli_options_mean_what_the_references_parser_says(hip_lib_host, name):
    """Where oracle/_ref is not built: the reference's string as tests/golden/ref_offline.npz holds it (oracle/gen_golden_ref_offline.py)."""
    o = E.build_parser().parse_args(ARGS[name].split() + ["-o", "x.264", "in_352x288.yuv"])
    p = mux.encoder_params(hip_lib_host, validate=False, width=352, height=288, **E.param_fields(o))
    if os.path.exists(REF_SO):
        want = reference_string(ARGS[name])
    else:
        with np.load(os.path.join(ROOT, "tests", "golden", "ref_offline.npz")) as g:
            want = str(g["p2s_cli_%s" % name])
    assert mux.param2string(hip_lib_host, p) == want


def test_raw_and_y4m_readers(tmp_path):
    w, h, n = 48, 32, 3
    fr = [synth.frame(w, h, t) for t in range(n)]
    raw = tmp_path / "clip_48x32.yuv"
    with open(raw, "wb") as f:
        for y, u, v in fr:
            f.write(y.tobytes()); f.write(u.tobytes()); f.write(v.tobytes())
    y4 = tmp_path / "clip.y4m"
    with open(y4, "wb") as f:
        f.write(b"YUV4MPEG2 W48 H32 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG\n")
        for k, (y, u, v) in enumerate(fr):
            f.write(b"FRAME\n" if k != 1 else b"FRAME Ip\n")          # a frame header may carry parameters (R/muxers.c:296-304)
            f.write(y.tobytes()); f.write(u.tobytes()); f.write(v.tobytes())
    a, b = E.open_inputs([str(raw)])[0], E.open_inputs([str(y4)])[0]
    c = E.open_inputs([str(raw), "48x32"])[0]
    assert (a.w, a.h, a.n, a.fps) == (48, 32, 3, None) and (b.w, b.h, b.n, b.fps) == (48, 32, 3, (30000, 1001)) and (c.w, c.h, c.n) == (48, 32, 3)
    for t in (2, 0, 1):
        for r in (a, b, c):
            for got, want in zip(r.read(t), fr[t]):
                assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        E.open_inputs([str(tmp_path / "nores.yuv")])
