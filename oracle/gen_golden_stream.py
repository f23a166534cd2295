"""TEST INFRASTRUCTURE -- regenerates tests/golden/stream_*.npz: the REFERENCE's whole encoder (frame queue, x264_slicetype_decide,
x264_ratecontrol_start, the slice loop with the entropy coder; oracle/ref_slice.c refslice_encode_stream) on the clips and options of
tests/test_gpu_stream.py (tests/stream_util.py) -- per coded frame the input number, slice type, QP and the slice_data() bytes -- and
tests/golden/stream_batch_{med,slow}.npz, the clips of tests/test_gpu_full_batch.py (tests/full_batch_util.py; bench.py's MED and SLOW flag sets) with each coded
frame's frame_num besides; those are written byte for byte the same on every run (save_npz).
Needs oracle/_ref/libx264ref.so (`make -C oracle ref`, i.e. /root/reference).

    python -m oracle.gen_golden_stream
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def save_npz(path, arrays):
    """np.savez_compressed without the time of day: entries in sorted order, every member dated 1980-01-01, so that regenerating a
    fixture reproduces the committed file byte for byte.  np.load reads it as any .npz."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main_batch():
    import full_batch_util as T
    for name in sorted(T.FLAGS):
        out = {}
        for i, a in enumerate(T.reference(name)):
            for k, v in a.items():
                out["c%d_%s" % (i, k)] = v
            print("batch", name, i, "".join("PBI"[int(t)] for t in a["frame_info"][:, 0]), [int(q) for q in a["frame_info"][:, 1]],
                  int(a["payload_len"].sum()), "bytes")
        save_npz(os.path.join(ROOT, "tests", "golden", "stream_batch_%s.npz" % name), out)


def main():
    main_batch()
    import look_cases as K
    import stream_util as T
    for name in sorted(T.CONFIGS):
        out = {}
        for i, c in enumerate(T.chains(name, T.SEEDS[name])):
            a = K.reference_records(c)
            for k in ("frame_info", "frame_info2", "payload", "payload_len"):
                out["c%d_%s" % (i, k)] = a[k]
            print(name, i, "".join("PBI"[int(t)] for t in a["frame_info"][:, 0]), [int(q) for q in a["frame_info"][:, 1]], int(a["payload_len"].sum()), "bytes")
        np.savez_compressed(os.path.join(ROOT, "tests", "golden", "stream_%s.npz" % name), **out)


if __name__ == "__main__":
    main()
