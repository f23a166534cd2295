"""The lossless raster kernels as the built code objects describe them (no GPU needed): they exist under names of their own -- so that the
lossy raster kernels stay the instantiations tests/test_build_resources.py counts -- and stay inside the resources of the kernels they
mirror: no spilled registers, at most 64 bytes of private segment (test_no_kernel_spills_registers holds them to that too), LDS within
24 KiB.  The lookahead's SAD kernels sit beside the SATD ones."""
import re

from kernel_meta import RASTER, kernel_metadata


def demangled_bools(name):
    """k_lossless_raster<RF, CH>: the two template arguments from the mangled name (ILb?ELb?EE)."""
    m = re.search(r"ILb([01])ELb([01])EE", name)
    return (int(m.group(1)), int(m.group(2))) if m else None


def test_lossless_raster_kernels_exist_under_their_own_names(tmp_path):
    md = kernel_metadata(tmp_path)
    ll = {k: v for k, v in md.items() if "k_lossless_raster" in k}
    # lock-step and chain-table launches, each without and with the RD refinement of subme 8-9
    assert sorted(demangled_bools(k) for k in ll) == [(0, 0), (0, 1), (1, 0), (1, 1)], sorted(ll)
    for k, v in ll.items():
        assert "k_slice_sweep" not in k
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] <= 64, (k, v)
        assert v["group_segment_fixed_size"] <= 24 * 1024, (k, v)
        rf = demangled_bools(k)[0]
        assert v["vgpr_count"] <= (512 if rf else 256), (k, v)      # the refinement variant: one wave per SIMD, the others two
    # no instantiation of the shared sweep with lossless AND the raster order is left under the old name
    assert not [k for k in md if "k_slice_sweep" in k and RASTER.search(k) and re.search(r"ILi\dELb1E", k)]


def test_lookahead_sad_kernels_exist(tmp_path):
    md = kernel_metadata(tmp_path)
    for name in ("k_look_cost_sad", "k_lookahead_intra_sad"):
        ks = [v for k, v in md.items() if name in k]
        assert len(ks) == 1, name
        assert ks[0]["vgpr_spill_count"] == 0 and ks[0]["private_segment_fixed_size"] <= 64, (name, ks[0])
