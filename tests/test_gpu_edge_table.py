"""GPU: x264hip_slice_sweep_chains -- the chain table's own kernels (frame_slice_rd_ch / _rf_ch / _ll_ch / _ll_rf_ch.hip) -- on pictures of
one to six macroblocks.  StreamEncoder cannot reach them at these sizes (x264hip_lookahead_cost_frames refuses mb_w <= 2 or mb_h <= 2), so
the launches are tests/table_util.py's.  Nine I / P chains = the nine contents of tests/edge_cases.py in one table; the lossy tables give
chain b the QP (8, 26, 51)[b % 3] and, in a second run, (1, 2, 3)[b % 3] -- lossy chains whose I slices are at QP 0 and whose levels
pass 3000 --, the lossless ones QP 0 throughout (a table is all-lossless or not at all).  Expected, bit for bit: the
CPU twin run at that chain's QP (pinned to the reference by tests/test_oracle_edge_chains.py); for lossless with the RD refinement,
which the twin does not code, the reference's digests in tests/golden/edge_chains.npz and the source planes."""
import numpy as np
import pytest

import edge_cases as E
from table_util import table_launch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kernel", list(E.TABLE))
@pytest.mark.parametrize("size", E.TABLE_SIZES, ids=E.size_id)
def test_chain_table_on_tiny_pictures(hip_lib, oracle_lib, cqm, size, kernel):
    check_table(hip_lib, cqm, size, kernel, False)


@pytest.mark.parametrize("kernel", [k for k, n in E.TABLE.items() if n in E.TABLE_LOSSY])
@pytest.mark.parametrize("size", E.TABLE_SIZES, ids=E.size_id)
def test_chain_table_on_tiny_pictures_at_qp_1_2_3(hip_lib, oracle_lib, cqm, size, kernel):
    check_table(hip_lib, cqm, size, kernel, True)


def check_table(hip_lib, cqm, size, kernel, low):
    name = E.TABLE[kernel]
    src, kw, ekw, frames = E.CONFIGS[name]
    qps = E.table_qps(name, low)
    clips = [E.clip(kind, size, frames) for kind in E.CONTENTS]
    out = table_launch(hip_lib, cqm, size, frames, None, None, None, dict(kw, **ekw), qps, clips=clips, arrays=E.DECISIONS)
    for b, (kind, qp) in enumerate(zip(E.CONTENTS, qps)):
        a = E.twin_chain(name, size, kind, qp if qp else None)
        gold = E.recorded(name, size, kind) if src == "ref" else None
        for f in range(frames):
            what = "%s (%s) %dx%d chain %d (%s, QP %d) frame %d" % (kernel, name, size[0], size[1], b, kind, qp, f)
            d = out[f]
            if a is not None:
                for k in E.DECISIONS:
                    got, want = d["state"][k][b], a[k][f]
                    assert np.array_equal(got.reshape(want.shape), want), "%s: %s differs first at %s" % (what, k, np.argwhere(got.reshape(want.shape) != want)[:3].tolist())
                assert d["payload"][b] == E.payload(a, f), "%s: payload differs (%d bytes, the twin %d)" % (what, len(d["payload"][b]), int(a["payload_len"][f]))
                for i, nm in enumerate("yuv"):
                    assert np.array_equal(d["fin"][i][b], a["fin_" + nm][f]), "%s: fin_%s" % (what, nm)
            else:
                assert E.md5(d["state"]["mb_type"][b]) == bytes(gold[1][f]), "%s: mb_type differs from the reference's" % what
                assert E.md5(np.frombuffer(d["payload"][b], np.uint8)) == bytes(gold[0][f]), "%s: payload (%d bytes) differs from the reference's" % (what, len(d["payload"][b]))
            if qp == 0:
                for i in range(3):
                    s = clips[b][i][f]
                    for k in ("rec", "fin"):
                        assert np.array_equal(d[k][i][b][:s.shape[0], :s.shape[1]], s), "%s: lossless %s plane %d is not the source" % (what, k, i)
