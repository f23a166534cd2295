"""Without a GPU: the chain-table CAVLC writer is part of the ABI (exported, and declared in include/x264hip_lookahead.h with the entry
structure the Python mirror has), and the command line front end accepts `--no-cabac` with CRF, B frames and scene cuts -- what it still
refuses is CAVLC with the RD levels."""
import ctypes as C
import os
import re

import pytest

from paths import ROOT
from x264_vs2008_amd import encode as E
from x264_vs2008_amd import mux, slice as sl


def test_cavlc_write_chains_is_exported_and_declared(hip_lib_host):
    for name in ("x264hip_cavlc_write_chains", "x264hip_chain_cavlc_bytes", "x264hip_cavlc_write_frame"):
        assert hasattr(hip_lib_host, name), "%s is not exported by libx264hip.so" % name
    head = open(os.path.join(ROOT, "include", "x264hip_lookahead.h")).read()
    assert re.search(r"int\s+x264hip_cavlc_write_chains\s*\(\s*x264hip_frame_ctx\s*\*\w+,\s*const\s+x264hip_chain_cavlc\s*\*\w+,\s*int\s+\w+,\s*void\s*\*\w+,\s*void\s*\*\w+\)", head)
    m = re.search(r"typedef struct \{([^}]*)\} x264hip_chain_cavlc;", head)
    assert m, "x264hip_chain_cavlc is not declared"
    fields = re.findall(r"(\w+)\s*;", m.group(1))
    assert fields == [f for f, _ in sl.ChainCavlc._fields_]
    assert C.sizeof(sl.ChainCavlc) == 24 and hip_lib_host.x264hip_chain_cavlc_bytes() >= C.sizeof(sl.ChainCavlc)


@pytest.mark.parametrize("args", ["--no-cabac --crf 23 --subme 5 --bframes 0", "--no-cabac --crf 23 --subme 5 --bframes 3 --b-adapt 1 --direct auto",
                                  "--no-cabac --qp 28 --subme 2 --bframes 2 --trellis 1"])
def test_command_line_accepts_no_cabac_with_the_frame_queue(hip_lib_host, args):
    o = E.build_parser().parse_args(args.split() + ["-o", "x.264", "in_96x80.yuv"])
    p = mux.encoder_params(hip_lib_host, width=96, height=80, **E.param_fields(o))
    assert not p.cabac and not p.trellis            # x264_validate_parameters: trellis goes off without CABAC
    assert E.needs_lookahead(p)
    E.check_built(p)                                # raises what the command line refuses


def test_command_line_still_refuses_cavlc_with_the_rd_levels(hip_lib_host):
    o = E.build_parser().parse_args("--no-cabac --crf 23 --subme 6".split() + ["-o", "x.264", "in_96x80.yuv"])
    p = mux.encoder_params(hip_lib_host, width=96, height=80, **E.param_fields(o))
    with pytest.raises(ValueError, match="RD levels"):
        E.check_built(p)
