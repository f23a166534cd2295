"""TEST INFRASTRUCTURE -- regenerates tests/golden/edge_chains.npz: what the REFERENCE's own loop (oracle/_ref/libx264ref.so) codes for
every (size, content, configuration) of tests/edge_cases.py -- pictures of one to six macroblocks, flat / saturated / full-range content.
Only recorded results are stored, as md5 digests (the scheme of ref_offline.npz): per configuration

  <name>_payload  uint8 [size][content][frame][16]   the payload of every frame (zeros: a chain without a writer),
  <name>_mb_type  uint8 [size][content][frame][16]   mb_type of every frame,
  <name>_whole    uint8 [size][content][array][16]   mv, ref, qp, cbp, fin_y, fin_u, fin_v over the chain (edge_cases.WHOLE),

and table_<name>_* for the lossy configurations of edge_cases.TABLE over TABLE_SIZES, every content at its chain-table QP (table_qps).

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
    out, chains = {}, []
    for name, (src, kw, ekw, frames) in E.CONFIGS.items():
        pay = np.zeros((len(E.SIZES), len(E.CONTENTS), frames, 16), np.uint8)
        mbt = np.zeros_like(pay)
        whole = np.zeros((len(E.SIZES), len(E.CONTENTS), len(E.WHOLE), 16), np.uint8)
        for i, size in enumerate(E.SIZES):
            for j, kind in enumerate(E.CONTENTS):
                a = E.reference_chain(name, size, kind)
                pay[i, j], mbt[i, j], whole[i, j] = E.digests(a, name)
                chains.append((name, size, kind, a["mb_type"].copy()))
                if kw["qp"] == 0:               # lossless: the reference reconstructs its source
                    y, u, v = E.clip(kind, size, frames)
                    for f, (disp, _) in enumerate(E.order_of(name)):
                        assert all(np.array_equal(a["fin_" + nm][f][:p.shape[1], :p.shape[2]], p[disp]) for nm, p in (("y", y), ("u", u), ("v", v))), (name, size, kind, f)
        out[name + "_payload"], out[name + "_mb_type"], out[name + "_whole"] = pay, mbt, whole
        print(name, src, "types", sorted({int(t) for c in chains if c[0] == name for t in np.unique(c[3])}))
    for name in E.TABLE.values():
        if E.CONFIGS[name][1]["qp"] == 0:       # all chains at QP 0: the configuration's own entries
            continue
        frames, qps = E.CONFIGS[name][3], E.table_qps(name)
        pay = np.zeros((len(E.TABLE_SIZES), len(E.CONTENTS), frames, 16), np.uint8)
        mbt = np.zeros_like(pay)
        whole = np.zeros((len(E.TABLE_SIZES), len(E.CONTENTS), len(E.WHOLE), 16), np.uint8)
        for i, size in enumerate(E.TABLE_SIZES):
            for j, kind in enumerate(E.CONTENTS):
                pay[i, j], mbt[i, j], whole[i, j] = E.digests(E.reference_chain(name, size, kind, qps[j]), name)
        out["table_" + name + "_payload"], out["table_" + name + "_mb_type"], out["table_" + name + "_whole"] = pay, mbt, whole
    bad = E.coverage_problems(chains)
    assert not bad, "the case list lost coverage:\n  " + "\n  ".join(bad)
    assert E.kinds_selected() == set(range(7)), E.kinds_selected()
    np.savez_compressed(E.FIXTURE, **out)
    print(E.FIXTURE, os.path.getsize(E.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
