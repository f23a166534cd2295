"""GPU: device-resident input through the encoders -- ChainEncoder.upload_device, a StreamEncoder whose fill() imports (a partial batch included)
and the command line's --input-csp / --vflip -- each against the same pictures fed through x264hip_picture_upload: the same bytes out."""
import os

import numpy as np
import pytest

import import_util as U
import look_cases as K
import stream_util as ts
from paths import ROOT
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import slice as sl
from x264_vs2008_amd import synth
from x264_vs2008_amd.frame import cqm_init
from x264_vs2008_amd.stream import StreamEncoder

pytestmark = pytest.mark.gpu


def _chain_run(hip_lib, w, h, clips, device, frames=4):
    """`frames` frames of a batch of 2 at subme 5 with the CABAC coder in the loop: per frame (slice type, qp), the payloads and the filtered reconstruction."""
    enc = sl.ChainEncoder(hip_lib, w, h, cqm_init(hip_lib), batch=2, qp=26, subme=5, me_method=1, n_refs=2, cabac=1, deblock=1, write=1)
    out, held = [], []
    try:
        for f in range(frames):
            if device:
                held.append([U.Surface(hip_lib, *clips[b][f], "nv12", "top_down", "w+13", 0, last=b) for b in range(2)])
                enc.upload_device([s.entry(b) for b, s in enumerate(held[-1])])
            else:
                for b in range(2):
                    enc.upload(*clips[b][f], b=b)
            stype, qp, _ = enc.encode_frame()
            enc.status()
            enc.sync()
            pays = enc.payloads()
            enc.finish_frame()
            enc.sync()
            fin = {(b, n): enc.ctx.download(enc.refs[0][0], n, padded=True, b=b) for b in range(2) for n in "yuv"}
            out.append(((stype, qp), pays, fin))
    finally:
        enc.close()
        for row in held:
            for s in row:
                s.free()
    return out


@pytest.mark.parametrize("size", [(48, 32), (208, 144)], ids=lambda s: "%dx%d" % s)
def test_chain_encoder_codes_the_same_from_device_surfaces(hip_lib, size):
    w, h = size
    clips = [[U.content(w, h, 3 * b, t) for t in range(4)] for b in range(2)]          # (3 * b: both chains the textured kind, their own content)
    a, b = _chain_run(hip_lib, w, h, clips, False), _chain_run(hip_lib, w, h, clips, True)
    assert len(a) == len(b) == 4
    for f, ((info_a, pay_a, fin_a), (info_b, pay_b, fin_b)) in enumerate(zip(a, b)):
        assert info_a == info_b, "frame %d: (slice type, qp) %s from upload, %s from upload_device" % (f, info_a, info_b)
        assert all(len(p) > 0 for p in pay_a)
        assert pay_a == pay_b, "frame %d: payloads differ (%s vs %s bytes)" % (f, [len(p) for p in pay_a], [len(p) for p in pay_b])
        for k in fin_a:
            assert np.array_equal(fin_a[k], fin_b[k]), "frame %d: reconstruction of element %d plane %s differs" % ((f,) + k)


def _lanes_run(hip_lib, w, h, clips, order, device):
    """An I P B B ... chain of a batch of 2 whose B frames run on a lane's own stream: per coded frame the payloads and, of a kept frame, the
    reconstruction.  Nothing synchronises between the picture's arrival and the sweep: with upload_device the lane's stream has to wait."""
    enc = sl.ChainEncoder(hip_lib, w, h, cqm_init(hip_lib), batch=2, qp=26, subme=5, me_method=1, n_refs=2, inter=0x113, intra=0x3, cabac=1, deblock=1, write=1,
                          bframes=2, lanes=1)
    out, held = [], []
    try:
        for disp, stype in order:
            if device:
                held.append([U.Surface(hip_lib, *clips[b][disp], "nv12", "vflip_flag", "w+1", 3, last=b) for b in range(2)])
                enc.upload_device([s.entry(b) for b, s in enumerate(held[-1])])
            else:
                for b in range(2):
                    enc.upload(*clips[b][disp], b=b)
            enc.encode_frame(stype=stype, disp=disp)
            enc.sync()
            enc.status()
            pays = enc.payloads()
            enc.finish_frame()
            enc.sync()
            fin = {} if stype == sl.SLICE_B else {(b, n): enc.ctx.download(enc.refs[0][0], n, padded=True, b=b) for b in range(2) for n in "yuv"}
            out.append((stype, pays, fin))
    finally:
        enc.close()
        for row in held:
            for s in row:
                s.free()
    return out


def test_chain_encoder_with_lanes_waits_for_the_import(hip_lib):
    """lanes=1, bframes=2: the B frames are swept on a stream of their own, which upload_device orders behind the import (upload synchronises)."""
    w, h, n = 96, 80, 7
    order = sl.coding_order(n, 0, 2)
    assert sum(st == sl.SLICE_B for _, st in order) >= 4
    clips = [[U.content(w, h, 3 * b, t) for t in range(n)] for b in range(2)]
    a, b = _lanes_run(hip_lib, w, h, clips, order, False), _lanes_run(hip_lib, w, h, clips, order, True)
    for f, ((st_a, pay_a, fin_a), (st_b, pay_b, fin_b)) in enumerate(zip(a, b)):
        assert st_a == st_b and all(len(p) > 0 for p in pay_a)
        assert pay_a == pay_b, "coded frame %d (slice type %d): payloads differ (%s vs %s bytes)" % (f, st_a, [len(p) for p in pay_a], [len(p) for p in pay_b])
        for k in fin_a:
            assert np.array_equal(fin_a[k], fin_b[k]), "coded frame %d: reconstruction of element %d plane %s differs" % ((f,) + k)


@pytest.mark.parametrize("size", [(10, 6), (2, 2)], ids=lambda s: "%dx%d" % s)
def test_encoder_below_one_macroblock_codes_its_coded_picture(hip_lib, size):
    """A picture below 16x16 is its one coded macroblock with the visible samples replicated: an I P P chain of it, fed by upload and by
    upload_device, gives the payloads and reconstructions of the 16x16 pictures that hold the replicated samples."""
    w, h = size
    small = [[U.content(w, h, 3 * b, t) for t in range(3)] for b in range(2)]
    padded = [[tuple(np.pad(p, ((0, (16 >> (i > 0)) - p.shape[0]), (0, (16 >> (i > 0)) - p.shape[1])), mode="edge") for i, p in enumerate(f)) for f in c] for c in small]
    want = _chain_run(hip_lib, 16, 16, padded, False, frames=3)
    for device in (False, True):
        got = _chain_run(hip_lib, w, h, small, device, frames=3)
        for f, ((info_a, pay_a, fin_a), (info_b, pay_b, fin_b)) in enumerate(zip(want, got)):
            assert info_a == info_b and all(len(p) > 0 for p in pay_a)
            assert pay_a == pay_b, "frame %d, device input %s: payloads differ from the 16x16 picture's" % (f, device)
            for k in fin_a:
                assert np.array_equal(fin_a[k], fin_b[k]), "frame %d, device input %s: reconstruction of element %d plane %s differs" % ((f, device) + k)


STREAM_CASE = "temporal_crf"          # the smallest CRF configuration with B frames of stream_util.CONFIGS (128x80, 12 pictures)


def _stream_run(hip_lib, cs, clips, limits, device):
    c, frames = cs[0], cs[0]["frames"]
    enc = StreamEncoder(hip_lib, c["w"], c["h"], cqm_init(hip_lib), batch=len(cs), limits=limits, crf=c["crf"], b_adapt=c["b_adapt"], bframe_bias=c["bframe_bias"],
                        keyint_min=c["keyint_min"], scenecut_threshold=c["scenecut_threshold"], pre_scenecut=c["pre_scenecut"],
                        qp=c["qp"], me_method=c["me"], me_range=16, subme=c["subme"], n_refs=c.get("n_refs", 2), inter=c.get("inter", 0x33), intra=0x3,
                        transform8x8=1, cabac=1, deblock=1, keyint=c["keyint"], mixed_refs=c.get("mixed_refs", 0), chroma_me=c.get("chroma_me", 1),
                        trellis=c.get("trellis", 0), psy_rd=c.get("psy_rd", 0.0), aq_mode=c["aq"], aq_strength=1.0, bframes=c["bframes"],
                        weightb=c["weightb"], direct_pred=c.get("direct_pred", 1), qp_min=0)
    got, records, held, partial = [[] for _ in cs], [], [], []

    def fill(pic, f):
        live = [b for b in range(len(cs)) if f < limits[b]]           # a chain that has run out of input is not named
        partial.append(len(live) < len(cs))
        if device:
            held.append([U.Surface(hip_lib, clips[b][0][f], clips[b][1][f], clips[b][2][f], "yv12", "vflip_flag", "w+1", 2, last=b) for b in live])
            enc.src_ctx.import_surfaces(pic, [s.entry(b) for b, s in zip(live, held[-1])])
        else:
            for b in live:
                enc.src_ctx.upload(pic, clips[b][0][f], clips[b][1][f], clips[b][2][f], b=b)

    try:
        fed, idle = 0, 0
        for _ in range(4 * frames + 40):
            coded = enc.step(fill if fed < frames else None)
            fed += fed < frames
            idle = 0 if coded else idle + (fed >= frames and enc.flushing)
            if idle >= 2:
                break
            if coded:
                enc.sync()
                enc.status()
                pl = enc.payloads()
                for cd in coded:
                    got[cd.chain].append((cd.frame, cd.slice_type, cd.qp, pl[cd.chain]))
                    records.append((cd.chain, cd.frame, cd.type, cd.slice_type, cd.qp, cd.f_qpm, cd.poc, cd.n_ref0, cd.n_ref1, cd.i_satd, int(cd.frame_num_reset),
                                    int(cd.direct_spatial), pl[cd.chain]))
    finally:
        enc.close()
        for row in held:
            for s in row:
                s.free()
    assert any(partial) and not all(partial)
    return got, records


def test_stream_encoder_fill_imports_a_partial_batch(hip_lib):
    """Two chains, the second one picture shorter: the last fill() names chain 0 only.  Fed by import_surfaces (YV12 | VFLIP) the encoder returns the
    Coded records and payloads it returns fed by upload, and chain 0's are the reference encoder's (the fixture the stream tests hold it to)."""
    cs = ts.chains(STREAM_CASE, ts.SEEDS[STREAM_CASE])[:2]
    frames = cs[0]["frames"]
    clips = [K.clip(c["w"], c["h"], frames, c["cut"], c["t0"], c["slow"]) for c in cs]
    limits = [frames, frames - 1]
    up, up_records = _stream_run(hip_lib, cs, clips, limits, False)
    dev, dev_records = _stream_run(hip_lib, cs, clips, limits, True)
    assert [len(g) for g in dev] == limits
    assert len(up_records) == len(dev_records) == sum(limits)
    for i, (a, b) in enumerate(zip(up_records, dev_records)):
        assert a[:-1] == b[:-1], "coded frame %d: %s fed by upload, %s fed by import_surfaces" % (i, a[:-1], b[:-1])
        assert a[-1] == b[-1], "coded frame %d (chain %d, input %d): payloads differ (%d vs %d bytes)" % (i, a[0], a[1], len(a[-1]), len(b[-1]))
    gold = np.load(os.path.join(ROOT, "tests", "golden", "stream_%s.npz" % STREAM_CASE))
    ts.check(dev[0], {k: gold["c0_" + k] for k in ("frame_info", "frame_info2", "payload", "payload_len")}, cs[0], "import-fed chain 0")


CLI = ["--qp", "26", "--subme", "5"]


@pytest.mark.parametrize("more", [[], ["--scenecut", "-1"]], ids=["frame_queue", "lock_step"])
@pytest.mark.parametrize("layout,vflip", [("nv12", False), ("yv12", True)], ids=["nv12", "yv12_vflip"])
def test_command_line_reads_other_layouts(hip_lib, tmp_path, layout, vflip, more):
    """--input-csp nv12, and --input-csp yv12 --vflip, on raw files of the same 6 pictures: the .264 of the default run on the I420 file.  With
    the default scene cut the frame queue's fill() imports, with --scenecut -1 the lock-step encoder's upload_device."""
    w, h, n = 96, 80, 6
    frames = [synth.frame(w, h, t) for t in range(n)]
    plain, other = tmp_path / ("clip_%dx%d.yuv" % (w, h)), tmp_path / ("clip_%dx%d.%s" % (w, h, layout))
    plain.write_bytes(b"".join(U.raw_frame(y, u, v, "i420", False) for y, u, v in frames))
    other.write_bytes(b"".join(U.raw_frame(y, u, v, layout, vflip) for y, u, v in frames))
    assert plain.read_bytes() != other.read_bytes() and plain.stat().st_size == other.stat().st_size == n * w * h * 3 // 2
    out_a, out_b = tmp_path / "a.264", tmp_path / "b.264"
    assert E.main(CLI + more + ["-o", str(out_a), str(plain)]) == 0
    assert E.main(CLI + more + ["--input-csp", layout] + (["--vflip"] if vflip else []) + ["-o", str(out_b), str(other)]) == 0
    a, b = out_a.read_bytes(), out_b.read_bytes()
    assert len(a) > 1000 and a == b, "the .264 differs: %d bytes from I420, %d from %s%s" % (len(a), len(b), layout, " bottom-up" if vflip else "")


@pytest.mark.parametrize("args,needle", [(["--input-csp", "nv12"], "--input-csp nv12"), (["--vflip"], "--vflip")], ids=["nv12", "vflip"])
def test_command_line_refuses_y4m_with_another_layout(hip_lib, tmp_path, args, needle):
    import mux_cases as M
    path = tmp_path / "clip.y4m"
    M.write_clip(str(path), 96, 80, 2, y4m=True)
    with pytest.raises(SystemExit) as ex:
        E.main(CLI + args + ["-o", str(tmp_path / "o.264"), str(path)])
    assert needle in str(ex.value) and "YUV4MPEG2" in str(ex.value)
    assert not (tmp_path / "o.264").exists()
