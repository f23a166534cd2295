"""TEST INFRASTRUCTURE -- regenerates tests/golden/ref_offline.npz: what the REFERENCE (oracle/_ref/libx264ref.so) answers for the cases
of the host tests that used to run only where that library is built, so that they hold the product to the reference everywhere:

  * p2s_mux_<name>, p2s_cli_<name>: x264_param2string after x264_param_parse of tests/mux_cases.py CLI / ARGS (tests/test_cpu_mux.py, tests/test_cpu_encode_cli.py);
  * rc<seed>_<what>: the md5 of the reference's payload of every frame and of its mb_type / mv / ref / qp / cbp arrays for the random chains
    of tests/test_oracle_random_chains.py (tests/fuzz_b.py);
  * live<seed>_head / _qavg / _mv: the reference encoder's records of tests/test_lookahead_host.py's further seeds (the look_host.npz layout);
  * post<seed>_give / _head / _qavg / _mv: the same without --pre-scenecut, with the attempts its post-encode scene cut gave up.

Needs oracle/_ref/libx264ref.so (`make -C oracle ref`, i.e. the reference's sources).

    python -m oracle.gen_golden_ref_offline
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fuzz_b                       # noqa: E402
import look_cases as K              # noqa: E402
import mux_cases as M               # noqa: E402
from oracle import hostpic          # noqa: E402
from oracle import refslice as rs   # noqa: E402
from paths import REF_SO            # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_offline.npz")


def param_string(pairs):
    """x264_param2string of the reference after x264_param_default + x264_param_parse(name, value) for every pair."""
    ref = hostpic.load_lazy(REF_SO)
    ref.x264_param2string.restype = C.c_void_p
    buf = C.create_string_buffer(16384)
    ref.x264_param_default(buf)
    for k, v in pairs:
        assert ref.x264_param_parse(buf, k.encode(), None if v is None else v.encode()) == 0, (k, v)
    return C.string_at(ref.x264_param2string(buf, 0)).decode()


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def chain_digests(b, frames):
    """What tests/test_oracle_random_chains.py compares, as md5s: the payload of every frame, then each decision array."""
    pay = [md5(b["payload"][f, :b["payload_len"][f]]) for f in range(frames)]
    return np.array(pay), {k: np.array(md5(b[k])) for k in fuzz_b.ARRAYS}


def look_arrays(recs, n):
    """tests/look_cases.py records in the layout of look_host.npz (oracle/gen_golden_look.py)."""
    head = np.array([[r["frame"], r["slice"], r["poc"], r["qp"], r["satd"], r["mv0"] is not None, r["mv1"] is not None] for r in recs], np.int32)
    mv = np.zeros((len(recs), 2, n, 2), np.int16)
    for i, r in enumerate(recs):
        for l in (0, 1):
            if r["mv%d" % l] is not None:
                mv[i, l] = r["mv%d" % l]
    return head, np.array([r["f_qp_avg"] for r in recs], np.float32), mv


def main():
    out = {}
    for name, pairs in M.CLI.items():
        out["p2s_mux_%s" % name] = np.array(param_string(pairs))
    for name, args in M.ARGS.items():
        out["p2s_cli_%s" % name] = np.array(M.reference_string(args))
    for seed in fuzz_b.SEEDS:
        w, h, frames, kind, kw, ekw, y, u, v = fuzz_b.config(seed)
        b = rs.run_reference2(rs.make_params(w, h, frames, **kw), rs.make_ext(**ekw), y, u, v)
        pay, arrs = chain_digests(b, frames)
        out["rc%d_payload" % seed] = pay
        for k, d in arrs.items():
            out["rc%d_%s" % (seed, k)] = d
        print("random chain", seed, kind)
    for seed in K.LIVE_SEEDS:
        c = K.config(seed)
        recs = K.records_of_reference(K.reference_records(c), c["frames"])
        out["live%d_head" % seed], out["live%d_qavg" % seed], out["live%d_mv" % seed] = look_arrays(recs, ((c["w"] + 15) // 16) * ((c["h"] + 15) // 16))
        print("lookahead", seed)
    for seed in K.POST_SEEDS:
        c = K.post_config(seed)
        a = K.reference_records(c)
        recs = K.records_of_reference(a, c["frames"])
        out["post%d_give" % seed] = np.array([int(a["stat"][f][3]) for f in range(c["frames"])], np.int32)
        out["post%d_head" % seed], out["post%d_qavg" % seed], out["post%d_mv" % seed] = look_arrays(recs, ((c["w"] + 15) // 16) * ((c["h"] + 15) // 16))
        print("post-encode scene cut", seed)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
