"""TEST INFRASTRUCTURE -- regenerates tests/golden/edge_chains.npz: what the REFERENCE's own loop (oracle/_ref/libx264ref.so) codes for
every (size, content, configuration) of tests/edge_cases.py -- pictures of one to six macroblocks, flat / saturated / full-range content.
Only recorded results are stored, as md5 digests (the scheme of ref_offline.npz): per configuration

  <name>_payload  uint8 [size][content][frame][16]   the payload of every frame (zeros: a chain without a writer),
  <name>_mb_type  uint8 [size][content][frame][16]   mb_type of every frame,
  <name>_whole    uint8 [size][content][array][16]   mv, ref, qp, cbp, fin_y, fin_u, fin_v over the chain (edge_cases.WHOLE),

table_<name>_* for the lossy configurations of edge_cases.TABLE over TABLE_SIZES, every content at its chain-table QP (table_qps), tablelow_<name>_*
the same at the low assignment (table_qps(name, low=True): QP 1, 2, 3), and for the LOW_QP configurations

  <name>_max_level  int32 [size][content]            the largest |level| of the chain (under CAVLC a lower bound where an 8x8-transform
                                                      block's levels are recorded incompletely, see tests/cavlc_host_util.py),

so that a failing GPU chain can be put into its writer branch without the reference.

The coverage conditions tests/test_oracle_edge_chains.py asserts on the twin are asserted here on the reference before the file is written.
Needs oracle/_ref/libx264ref.so (`make -C oracle ref`, i.e. the reference's sources).

    python -m oracle.gen_golden_edge
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edge_cases as E              # noqa: E402


def main():
    out, chains, low = {}, [], []
    for name, (src, kw, ekw, frames) in E.CONFIGS.items():
        pay = np.zeros((len(E.SIZES), len(E.CONTENTS), frames, 16), np.uint8)
        mbt = np.zeros_like(pay)
        whole = np.zeros((len(E.SIZES), len(E.CONTENTS), len(E.WHOLE), 16), np.uint8)
        for i, size in enumerate(E.SIZES):
            for j, kind in enumerate(E.CONTENTS):
                a = E.reference_chain(name, size, kind)
                pay[i, j], mbt[i, j], whole[i, j] = E.digests(a, name)
                chains.append((name, size, kind, a["mb_type"].copy()))
                if name in E.LOW_QP:
                    low.append((name, size, kind, a["mb_type"].copy(), a["qp"].copy(), E.max_level(a)))
                if kw["qp"] == 0:               # lossless: the reference reconstructs its source
                    y, u, v = E.clip(kind, size, frames)
                    for f, (disp, _) in enumerate(E.order_of(name)):
                        assert all(np.array_equal(a["fin_" + nm][f][:p.shape[1], :p.shape[2]], p[disp]) for nm, p in (("y", y), ("u", u), ("v", v))), (name, size, kind, f)
        out[name + "_payload"], out[name + "_mb_type"], out[name + "_whole"] = pay, mbt, whole
        if name in E.LOW_QP:
            out[name + "_max_level"] = np.array([c[5] for c in low if c[0] == name], np.int32).reshape(len(E.SIZES), len(E.CONTENTS))
            print(name, "largest |level| per size", out[name + "_max_level"].max(1).tolist(), "QPs %d..%d" % (min(c[4].min() for c in low if c[0] == name),
                                                                                                            max(c[4].max() for c in low if c[0] == name)))
        print(name, src, "types", sorted({int(t) for c in chains if c[0] == name for t in np.unique(c[3])}))
    for name, is_low in [(n, l) for l in (False, True) for n in E.TABLE_LOSSY]:      # (a lossless table is all chains at QP 0: the configuration's own entries)
        frames, qps = E.CONFIGS[name][3], E.table_qps(name, is_low)
        pay = np.zeros((len(E.TABLE_SIZES), len(E.CONTENTS), frames, 16), np.uint8)
        mbt = np.zeros_like(pay)
        whole = np.zeros((len(E.TABLE_SIZES), len(E.CONTENTS), len(E.WHOLE), 16), np.uint8)
        for i, size in enumerate(E.TABLE_SIZES):
            for j, kind in enumerate(E.CONTENTS):
                pay[i, j], mbt[i, j], whole[i, j] = E.digests(E.reference_chain(name, size, kind, qps[j]), name)
        pre = "tablelow_" if is_low else "table_"
        out[pre + name + "_payload"], out[pre + name + "_mb_type"], out[pre + name + "_whole"] = pay, mbt, whole
    bad = E.coverage_problems(chains) + E.low_qp_problems(low)
    assert not bad, "the case list lost coverage:\n  " + "\n  ".join(bad)
    assert E.kinds_selected() == set(range(7)), E.kinds_selected()
    np.savez_compressed(E.FIXTURE, **out)
    print(E.FIXTURE, os.path.getsize(E.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
