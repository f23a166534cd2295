"""TEST INFRASTRUCTURE -- regenerates tests/golden/cavlc_*.npz: the slice_data() bytes the REFERENCE's CAVLC writer
(x264_macroblock_write_cavlc inside oracle/ref_slice.c's loop, refslice_encode_chain2 with cabac = 0) produces for the chains of
tests/test_gpu_cavlc.py (tests/cavlc_util.py), and tests/golden/cavlc_batch_uf.npz: the clips of tests/test_gpu_full_batch.py's wavefront chains (tests/full_batch_util.py; (bench.py --preset
cif's flag set), written byte for byte the same on every run.  Needs oracle/_ref/libx264ref.so.

    python -m oracle.gen_golden_cavlc
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main_batch():
    import full_batch_util as T
    from oracle.gen_golden_stream import save_npz
    from oracle import refslice as rs
    c = T.LOCK_WAVE
    out = {}
    for i, t0 in enumerate(T.LOCK_T0):
        a = T.cavlc_reference(c, rs.clip(c["w"], c["h"], c["frames"], t0))
        out["c%d_payload" % i], out["c%d_payload_len" % i] = a["payload"], a["payload_len"]
        print("batch", i, [int(n) for n in a["payload_len"]])
    save_npz(os.path.join(ROOT, "tests", "golden", "cavlc_batch_uf.npz"), out)


def main():
    main_batch()
    import cavlc_util as T
    for name in sorted(T.CONFIGS):
        _, pays, a = T.reference(T.CONFIGS[name])
        types = [int(np.bincount(a["mb_type"][f].astype(np.int64) & 31, minlength=8)[6]) for f in range(len(pays))]
        np.savez_compressed(os.path.join(ROOT, "tests", "golden", "cavlc_%s.npz" % name), payload=a["payload"], payload_len=a["payload_len"])
        print(name, [len(p) for p in pays], "skips per frame", types)


if __name__ == "__main__":
    main()
