"""CPU: the C-ABI library loads and exports every symbol include/*.h declares
(no compute, no GPU), host-side helpers, and the N > 1 frame-sharding path on
two gloo ranks."""
import ast
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from paths import ROOT


HEADERS = ("x264hip.h", "x264hip_lookahead.h", "x264hip_stream.h")
RAW_TYPEDEFS = {"x264hip_frame_stat": 32}          # the typedef structs Python reads as raw bytes (stream.py, through numpy) and mirrors by no record: name -> sizeof
STRUCT = r"typedef\s+struct\s*\w*\s*\{.*?\}\s*(\w+)\s*;"


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _class(decl, named):
    """The class of a return type, or of a parameter written with its name (named), as abi.PROTOTYPES spells it: a * or [ makes a pointer,
    anything else is int, size_t, float or (a return type) void.  Any other spelling is an error, not a guess."""
    if "*" in decl or "[" in decl:
        return "s" if not named and decl.replace("*", " * ").split() == ["const", "char", "*"] else "p"
    words = decl.split()[:-1] if named else decl.split()
    assert len(words) == 1 and words[0] in ("int", "size_t", "float") + (() if named else ("void",)), "no class for %r" % decl
    return {"int": "i", "size_t": "z", "float": "f", "void": "v"}[words[0]]


def _declarations(name):
    """{function: "return:parameters"} of the functions a header declares, in the notation of abi.PROTOTYPES."""
    src = re.sub(STRUCT, "", _header(name), flags=re.S)
    out = {}
    for ret, fn, params in re.findall(r"([\w \t\*]+?)\b(x264(?:hip)?_\w+)\s*\(([^;{()]*)\)\s*;", src):
        assert fn not in out, fn
        out[fn] = _class(ret, False) + ":" + "".join(_class(q, True) for q in params.split(",") if params.strip() != "void")
    return out


def test_library_exports_every_declared_symbol():
    from x264_vs2008_amd import lib as L
    if not os.path.exists(L.SO_PATH):
        L.build()
    lib = L.open_library()
    for header in HEADERS:
        declared = sorted(_declarations(header))
        assert len(declared) > (30 if header == "x264hip.h" else 8)
        missing = [n for n in declared if not hasattr(lib, n)]
        assert not missing, "declared in include/%s but not exported: %s" % (header, missing)


def test_prototype_table_is_the_headers():
    """abi.PROTOTYPES (what open_library() declares to ctypes) against include/*.h: exactly the declared functions, each with the declared
    return type, parameter count and parameter classes."""
    from x264_vs2008_amd.abi import PROTOTYPES
    declared = {}
    for header in HEADERS:
        d = _declarations(header)
        assert not set(d) & set(declared)
        declared.update(d)
    assert len(declared) > 100 and {v[0] for v in declared.values()} == set("ivpzsf")
    assert sorted(PROTOTYPES) == sorted(declared), sorted(set(PROTOTYPES) ^ set(declared))
    wrong = {n: (PROTOTYPES[n], declared[n]) for n in declared if PROTOTYPES[n] != declared[n]}
    assert not wrong, "function: (table, header) %s" % wrong


def test_records_match_header_layouts(tmp_path):
    """Every ctypes record of abi.RECORDS against its C typedef: sizeof, and offsetof / size of every field by name, printed by one C program
    generated from the records.  And the other way round: every typedef struct of the headers has a record or is listed in RAW_TYPEDEFS."""
    from x264_vs2008_amd import tables                     # registers the seven records of x264hip_tables.h
    from x264_vs2008_amd.abi import RECORDS
    assert tables.PixelTable in RECORDS.values()
    typedefs = [n for h in HEADERS + ("x264hip_tables.h",) for n in re.findall(STRUCT, _header(h), flags=re.S)]
    assert len(typedefs) == len(set(typedefs)) > 30
    assert not set(RECORDS) & set(RAW_TYPEDEFS)
    assert sorted(typedefs) == sorted(set(RECORDS) | set(RAW_TYPEDEFS)), "typedef structs without a record / records without a typedef: %s" % sorted(set(typedefs) ^ (set(RECORDS) | set(RAW_TYPEDEFS)))
    lines, want = [], {}
    for cname in RAW_TYPEDEFS:
        lines.append('printf("%s %%zu 0\\n", sizeof(%s));' % (cname, cname))
        want[cname] = (RAW_TYPEDEFS[cname], 0)
    for cname, rec in RECORDS.items():
        lines.append('printf("%s %%zu 0\\n", sizeof(%s));' % (cname, cname))
        want[cname] = (C.sizeof(rec), 0)
        for field in rec._fields_:
            f = field[0]
            lines.append('printf("%s.%s %%zu %%zu\\n", sizeof(((%s *)0)->%s), offsetof(%s, %s));' % (cname, f, cname, f, cname, f))
            want["%s.%s" % (cname, f)] = (getattr(rec, f).size, getattr(rec, f).offset)
    prog = "#include <stdio.h>\n#include <stddef.h>\n" + "".join('#include "%s"\n' % h for h in HEADERS) + "int main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n"
    src, exe = tmp_path / "layout.c", tmp_path / "layout.bin"
    src.write_text(prog)
    subprocess.run(["gcc", str(src), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        key, size, offset = line.split()
        got[key] = (int(size), int(offset))
    assert len(got) == len(want) > 400
    wrong = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not wrong, "record or field: ((size, offset) in ctypes, in C) %s" % wrong


def test_every_call_site_passes_the_declared_argument_count():
    """A wrong count raises only when the call runs, and most calls run only on a GPU: read them here.  Every call of a declared function in
    the package, the tests, bench.py and __graft_entry__.py is positional, without star-arguments, and has the declared arity."""
    from x264_vs2008_amd.abi import PROTOTYPES
    files = glob.glob(os.path.join(ROOT, "x264_vs2008_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tests", "*.py")) + \
        [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    bad, n = [], 0
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for call in (n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in PROTOTYPES):
            n += 1
            arity = len(PROTOTYPES[call.func.attr].split(":")[1])
            if call.keywords or any(isinstance(a, ast.Starred) for a in call.args) or len(call.args) != arity:
                bad.append("%s:%d %s takes %d positional arguments" % (os.path.relpath(path, ROOT), call.lineno, call.func.attr, arity))
    assert n > 200, n
    assert not bad, "\n  ".join(bad)


def test_bare_integer_address_is_passed_at_full_width():
    """What the prototypes are for: without them ctypes passes a Python integer as a 32-bit C int, and an address above 2^32 arrives cut in
    half.  x264hip_cost_mv_table is host C that writes through its third argument."""
    from x264_vs2008_amd import lib as L
    from x264_vs2008_amd.slice import COST_SPAN
    lib = L.open_library()
    n = 2 * COST_SPAN + 1
    big, want = np.zeros(1 << 22, np.int16), np.zeros(n, np.int16)           # (an allocation this large is mapped, far above 2^32)
    assert big.ctypes.data >> 32, "the buffer's address fits 32 bits: the test would not see a truncation"
    lib.x264hip_cost_mv_table(4, COST_SPAN, want.ctypes.data_as(C.c_void_p))
    lib.x264hip_cost_mv_table(4, COST_SPAN, big.ctypes.data)
    assert want.any() and np.array_equal(big[:n], want) and not big[n:].any()
    with pytest.raises(C.ArgumentError):
        lib.x264hip_cost_mv_table(4.0, COST_SPAN, want.ctypes.data_as(C.c_void_p))


def test_init_fails_loudly_without_gpu_or_inits_with_one():
    """No CPU fallback: without a device x264hip_init returns < 0 with a message and the
    table fillers refuse to fill; with a device it returns 0."""
    from x264_vs2008_amd import lib as L
    from x264_vs2008_amd.tables import PixelTable
    lib = L.open_library()
    n = lib.x264hip_device_count()
    cfg = L.Cfg(0, 0)
    rc = lib.x264hip_init(C.byref(cfg))
    if n == 0:
        assert rc < 0 and lib.x264hip_last_error()
        t = PixelTable()
        assert lib.x264_pixel_init_hip(C.byref(t)) == -1
        assert not any(bool(f) for f in t.sad)
    else:
        assert rc == 0


def test_cost_mv_table_properties():
    from x264_vs2008_amd.frame import cost_mv_table
    t = cost_mv_table(4, 64).astype(np.int64)
    assert t[64] == int(4 * 0.718 + 0.5) and np.array_equal(t, t[::-1]) and (np.diff(t[64:]) >= 0).all()


def test_gop_sharding_covers_every_frame_once():
    from x264_vs2008_amd import shard
    for n, k, w in ((100, 12, 4), (24, 250, 8), (97, 10, 3), (8, 1, 8)):
        seen = sorted(f for r in range(w) for f in shard.frames_for_rank(n, k, r, w))
        assert seen == list(range(n))
        for r in range(w):
            for a, b in shard.gops_for_rank(n, k, r, w):
                assert a % k == 0 and b - a <= k


WORKER = r'''
import os, sys
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from x264_vs2008_amd import shard
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
mine = shard.frames_for_rank(1000, 24, rank, world)
mask = torch.zeros(1000, dtype=torch.int32); mask[mine] = 1
dist.all_reduce(mask)                                   # every frame owned exactly once across ranks
t = torch.tensor([0.5 + rank], dtype=torch.float64); dist.all_reduce(t, op=dist.ReduceOp.MAX)   # bench.py's timing reduce
dist.barrier()
assert int(mask.min()) == 1 and int(mask.max()) == 1 and float(t[0]) == world - 0.5
print("rank", rank, "ok", len(mine))
dist.destroy_process_group()
'''


def test_two_rank_gloo_sharding(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("ok" in o for o in outs)


def test_cost_mv_table_built_in_c_matches_twin_and_numpy(oracle_lib):
    """p_cost_mv feeds every motion-vector decision and is float arithmetic in the reference (R/encoder/analyse.c:182-198).  The
    product builds it in the library's host C (x264hip_cost_mv_table, the reference's expression, -ffp-contract=off); it must equal
    the twin's C table (oracle/slice_oracle.c:s_load_cost_mv -- the twin is pinned to the reference's decisions on thousands of
    chains) and the NumPy restatement in frame.py, for every QP over the full +-2*4*2048 span."""
    import ctypes as C
    import numpy as np
    from x264_vs2008_amd import lib as L
    from x264_vs2008_amd.frame import cost_mv_table
    from x264_vs2008_amd.slice import COST_SPAN, LAMBDA_TAB
    lib = L.open_library()
    oracle_lib.x264o_cost_mv_row.restype = C.c_void_p
    for qp in range(52):
        got = np.zeros(2 * COST_SPAN + 1, np.int16)
        lib.x264hip_cost_mv_table(LAMBDA_TAB[qp], COST_SPAN, got.ctypes.data_as(C.c_void_p))
        twin = np.ctypeslib.as_array((C.c_int16 * (2 * COST_SPAN + 1)).from_address(oracle_lib.x264o_cost_mv_row(qp)))
        assert np.array_equal(got, twin), qp
        assert np.array_equal(got.view(np.uint16), cost_mv_table(LAMBDA_TAB[qp], COST_SPAN)), qp


def test_nal_encode_matches_reference():
    """x264hip_nal_encode (host C of the library) against the reference's own x264_nal_encode (oracle/_ref, built here from the
    reference's sources) on payloads full of the byte patterns emulation prevention exists for; where the reference library is
    absent, against the rule's statement in ITU-T H.264 7.4.1 (a 0x03 before any byte <= 3 that follows two zeros)."""
    import ctypes as C
    import os
    from x264_vs2008_amd import lib as L

    lib = L.open_library()
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libx264ref.so")
    ref = None
    if os.path.exists(ref_so):
        from oracle import refslice as rs
        ref = rs.reference_lib()

    class Nal(C.Structure):                      # x264_nal_t, R/x264.h:395-403
        _fields_ = [("i_ref_idc", C.c_int), ("i_type", C.c_int), ("i_payload", C.c_int), ("p_payload", C.c_void_p)]

    r = np.random.default_rng(5)
    for trial in range(60):
        n = int(r.integers(0, 400))
        pay = r.choice(np.array([0, 0, 0, 1, 2, 3, 4, 255], np.uint8), n) if trial % 2 else r.integers(0, 256, n).astype(np.uint8)
        pay = np.ascontiguousarray(pay)
        ref_idc, typ, annexb = int(r.integers(0, 4)), int(r.choice([1, 5, 6, 7, 8])), int(r.integers(0, 2))
        got = np.zeros(5 + n * 3 // 2 + 8, np.uint8)
        m = lib.x264hip_nal_encode(got.ctypes.data_as(C.c_void_p), annexb, ref_idc, typ, pay.ctypes.data_as(C.c_void_p), n)
        if ref is not None:
            want = np.zeros_like(got)
            size = C.c_int(0)
            nal = Nal(ref_idc, typ, n, pay.ctypes.data)
            ref.x264_nal_encode(want.ctypes.data_as(C.c_void_p), C.byref(size), annexb, C.byref(nal))
            assert m == size.value and np.array_equal(got[:m], want[:m]), trial
        out, zeros = ([0, 0, 0, 1] if annexb else []) + [(ref_idc << 5) | typ], 0
        for v in pay.tolist():
            if zeros == 2 and v <= 3:
                out.append(3); zeros = 0
            zeros = zeros + 1 if v == 0 else 0
            out.append(v)
        assert got[:m].tolist() == out, trial


from x264_vs2008_amd.frame import JVT4I, JVT4P, JVT8I, JVT8P          # the standard's default scaling lists (--cqm jvt)


def test_cqm_init_in_library_matches_reference_tables(oracle_lib):
    """x264hip_cqm_init (the library's host C restatement of x264_cqm_init, R/common/set.c:68-168) against the tables the REFERENCE's
    x264_cqm_init produced (tests/golden/cqm_flat.npz, cqm_jvt.npz: oracle/gen_golden_cqm.py), flat and JVT matrices, every QP; the
    unquant tables against the library's older x264hip_unquant_table and the twin's x264o_cqm_unquant."""
    import ctypes as C
    from x264_vs2008_amd import lib as L
    from x264_vs2008_amd.frame import cqm_init
    lib = L.open_library()
    for name, lists, qp_min in (("cqm_flat", None, 0), ("cqm_jvt", [JVT4I, JVT4P, JVT4I, JVT4P, JVT8I, JVT8P], 6)):
        t = cqm_init(lib, lists, qp_min=qp_min)
        with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) as z:
            for k in z.files:
                assert np.array_equal(t[k], z[k]), (name, k)
        preset = int(lists is not None)
        for cat in range(4):
            for qp in range(52):
                unq = np.zeros(16, np.int32)
                oracle_lib.x264o_cqm_unquant(preset, cat, qp, 0, unq.ctypes.data_as(C.c_void_p))
                assert np.array_equal(unq, t["unquant4_mf"][cat, qp]), (name, cat, qp)
        for cat in range(2):
            for qp in range(52):
                unq = np.zeros(64, np.int32)
                oracle_lib.x264o_cqm_unquant(preset, cat, qp, 1, unq.ctypes.data_as(C.c_void_p))
                assert np.array_equal(unq, t["unquant8_mf"][cat, qp]), (name, cat, qp)
    with pytest.raises(RuntimeError, match="overflow"):            # the JVT matrices below QP 6: "Quantization overflow", set.c:160-166
        cqm_init(lib, [JVT4I, JVT4P, JVT4I, JVT4P, JVT8I, JVT8P], qp_min=0)


def test_generated_cabac_tables_are_one_file():
    """oracle/cabac_tables.h (twin) and csrc/cabac_tables.h (product) are both written by oracle/gen_cabac_tables.py: the data must not drift."""
    import re
    def body(path):
        with open(path) as f:
            return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S).split()
    a, b = body(os.path.join(ROOT, "oracle", "cabac_tables.h")), body(os.path.join(ROOT, "x264_vs2008_amd", "csrc", "cabac_tables.h"))
    strip = lambda toks: [t for t in toks if t not in ("static", "__device__", "const", "__constant__")]
    ints = lambda toks: re.findall(r"-?\d+", " ".join(toks))
    assert ints(strip(a)) == ints(strip(b))


def test_encode_clip_refuses_what_it_cannot_shard():
    from x264_vs2008_amd import shard
    with pytest.raises(ValueError):
        shard.encode_clip(None, None, [(np.zeros((16, 16), np.uint8),) * 3], 4, lanes=1)
