"""The command line front end (x264_vs2008_amd/encode.py) without a GPU: its option parser against the REFERENCE's own x264_param_parse fed the
same options (x264_param2string of both, before validation), and the raw I420 / YUV4MPEG2 readers (R/muxers.c)."""
import ctypes as C
import os

import numpy as np
import pytest

from x264_vs2008_amd import encode as E
from x264_vs2008_amd import mux, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libx264ref.so")

ARGS = {
    "UF": "--qp 26 --no-cabac --me dia --subme 0 --partitions none --no-deblock --aq-mode 0 --scenecut -1 --ref 1 --bframes 0 --b-adapt 0",
    "MED": "--crf 23 --ref 3 --bframes 3 --b-adapt 1 --me hex --subme 7 --8x8dct --partitions p8x8,b8x8,i8x8,i4x4 --trellis 1 --weightb --mixed-refs --direct spatial",
    "SLOW": "--crf 23 --ref 5 --bframes 3 --b-adapt 2 --me umh --subme 8 --8x8dct --partitions p8x8,b8x8,i8x8,i4x4 --trellis 1 --weightb --mixed-refs --direct auto --pre-scenecut",
    "misc": "--qp 31 --ref 4 --bframes 2 --b-bias 10 --me esa --merange 24 --subme 9 --psy-rd 0.4:0.2 --trellis 2 --deblock=-1:2 --nr 100 --cqm jvt --chroma-qp-offset 3 "
            "--keyint 48 --min-keyint 6 --scenecut 30 --ipratio 1.2 --pbratio 1.5 --no-chroma-me --no-dct-decimate --deadzone-inter 12 --deadzone-intra 7 --partitions all",
    "crf_misc": "--crf 18.5 --qcomp 0.75 --qpmin 12 --qpmax 44 --qpstep 6 --aq-strength 0.7 --bframes 1 --no-cabac --no-fast-pskip --deblock 2 --psy-rd 0.8 --direct temporal",
}


def reference_string(args):
    from oracle import hostpic
    ref = hostpic.load_lazy(REF_SO)
    ref.x264_param2string.restype = C.c_void_p
    buf = C.create_string_buffer(16384)
    ref.x264_param_default(buf)
    toks = args.split()
    i = 0
    while i < len(toks):
        name = toks[i][2:]
        val = None
        if "=" in name:
            name, val = name.split("=", 1)
        elif i + 1 < len(toks) and not toks[i + 1].startswith("--"):
            val = toks[i + 1]
            i += 1
        i += 1
        assert ref.x264_param_parse(buf, name.encode(), None if val is None else val.encode()) == 0, (name, val)
    return C.string_at(ref.x264_param2string(buf, 0)).decode()


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
