"""What the built library's kernels say about themselves (no GPU needed): the AMDGPU metadata notes of every gfx950 kernel in
libx264hip.so, and the mangled-name patterns that tell the instantiations of the macroblock sweep apart (tests/test_build_resources.py,
tests/test_lossless_build_resources.py)."""
import os
import re
import shutil
import subprocess

import pytest

from paths import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_metadata(tmp_path):
    so = os.path.join(ROOT, "x264_vs2008_amd", "libx264hip.so")
    if not os.path.exists(so):
        import sys
        sys.path.insert(0, ROOT)
        from x264_vs2008_amd import lib as L
        L.build()                                        # hipcc cross-compiles without a GPU
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump")
    shutil.copy(so, tmp_path / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    out = {}
    for f in sorted(os.listdir(tmp_path)):
        if not f.endswith("gfx950"):
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name:
                out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count|group_segment_fixed_size):\s+(\d+)", blk)}
    return out


RASTER = re.compile(r"ILi\dELb[01]ELb1ELb[01]ELb[01]ELb[01]ELb[01]EEv")      # k_slice_sweep<WPE, LL, RD = true, BS, TD, RF, CH>
REFINE = re.compile(r"ILi\dELb[01]ELb1ELb[01]ELb[01]ELb1ELb[01]EEv")         # ... with the RD refinement of subme 8-9 (RF = true)
TABLE = re.compile(r"ILi\dELb[01]ELb1ELb[01]ELb[01]ELb[01]ELb1EEv")           # ... launched from a chain table (CH = true)
