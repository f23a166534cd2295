"""Helper of tests/test_gpu_psy_trellis.py: a ChainEncoder whose lock-step launches go through the chain table instead.

tests/table_util.table_launch builds its table by hand and knows I and P slices only.  ViaTable is a stand-in for the library handle: everything
is the library's own, except that x264hip_slice_sweep_frame becomes x264hip_slice_sweep_chains with one entry per batch element over the very
records ChainEncoder built for the lock-step launch (source, reference lists, slice parameters with their x264hip_slice_rd / x264hip_slice_b,
states).  So a B chain in coding order -- reference lists, list-1 state, direct prediction, weights -- reaches the chain-table kernels exactly as
slice_util.run_chain2 would have run it through the lock-step ones."""
import ctypes as C

import numpy as np

from x264_vs2008_amd.frame import DeviceArray
from x264_vs2008_amd.stream import ChainSweep


class ViaTable:
    def __init__(self, lib, batch):
        self._lib, self._batch = lib, batch
        self._bytes = lib.x264hip_chain_sweep_bytes() * batch
        self._host, self._dev = None, None
        self.launches = 0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def x264hip_slice_sweep_frame(self, h, fenc, refs, n_refs, recon, params, l0, out):
        lib, B = self._lib, self._batch
        if self._host is None:
            self._host, self._dev = lib.x264hip_host_alloc(self._bytes), DeviceArray(lib, (self._bytes,), np.uint8)

        def addr(r):
            return C.addressof(r._obj) if r is not None else None
        entries = (ChainSweep * B)()
        for b in range(B):
            entries[b] = ChainSweep(chain=b, fenc=addr(fenc), refs=C.cast(refs, C.c_void_p) if refs else None, n_refs=n_refs, recon=addr(recon),
                                    params=addr(params), l0=addr(l0), out=addr(out))
        rc = lib.x264hip_mb_state_clear_progress(h, out)
        if rc:
            return rc
        self.launches += 1
        return lib.x264hip_slice_sweep_chains(h, entries, B, self._host, self._dev.p)

    def free(self):
        """After the encoder is closed (its context synchronised)."""
        if self._host is not None:
            self._dev.free()
            self._lib.x264hip_host_free(self._host)
            self._host = None
