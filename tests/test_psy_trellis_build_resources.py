"""The psy-trellis kernels of the raster sweep, as the code objects describe themselves (no GPU needed): kernels of their own name
(k_psy_raster<BS, TD, RF, CH>) for every launch the lossy raster sweep has, without private memory.

Without the feature there is no such kernel and the first assertion fails."""
import re

from kernel_meta import kernel_metadata

PSY = re.compile(r"k_psy_rasterILb([01])ELb([01])ELb([01])ELb([01])EEv")
# (BS, TD, RF, CH): lock-step I / P, with the refinement, the extended B kernel (both kinds of lock-step B launch go there), and the chain-table three
WANT = {(0, 0, 0, 0), (0, 0, 1, 0), (1, 1, 0, 0), (0, 0, 0, 1), (0, 0, 1, 1), (1, 1, 0, 1)}


def test_psy_trellis_kernels_exist_under_their_own_name_without_private_memory(tmp_path):
    md = kernel_metadata(tmp_path)
    psy = {k: v for k, v in md.items() if "k_psy_raster" in k}
    got = {}
    for k, v in psy.items():
        m = PSY.search(k)
        assert m and "k_slice_sweep" not in k, k
        got[tuple(int(x) for x in m.groups())] = v
    assert set(got) == WANT and len(psy) == len(WANT), sorted(psy)
    for (bs, td, rf, ch), v in got.items():
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] <= 64, ((bs, td, rf, ch), v)
        assert v["group_segment_fixed_size"] <= 24 * 1024, ((bs, td, rf, ch), v)
        # one wave per SIMD was chosen for all six (amdgpu_waves_per_eu(1): held to 256 registers three of them spilled): a whole SIMD's register file
        assert v["vgpr_count"] <= 512, ((bs, td, rf, ch), v)
