"""hipMalloc / hipMemcpy / streams through the HIP runtime libsm_hip.so links.

The tests that hand the library caller-owned device buffers and caller-owned
streams use this instead of torch: a second HIP runtime initialised after the
library's finds no GPU, so nothing here (nor its importers) imports torch.
Import schwingermodel_amd first: it loads the runtime this module binds to.
"""
import ctypes

import numpy as np

H2D, D2H = 1, 2  # hipMemcpyHostToDevice, hipMemcpyDeviceToHost

# Every byte 0xFF: a quiet NaN with all payload bits set, as float64. No kernel
# here produces it, so a word that still holds it after a call was not written.
POISON = np.uint64(0xFFFFFFFFFFFFFFFF)


class Hip:
    def __init__(self):
        vp = ctypes.c_void_p
        self.rt = rt = ctypes.CDLL("libamdhip64.so.7")
        rt.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
        rt.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
        rt.hipFree.argtypes = [vp]
        rt.hipDeviceSynchronize.argtypes = []
        rt.hipStreamCreate.argtypes = [ctypes.POINTER(vp)]
        rt.hipStreamSynchronize.argtypes = [vp]
        rt.hipStreamDestroy.argtypes = [vp]
        self._owned = []

    # ---- memory ---------------------------------------------------------------
    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.rt.hipMalloc(ctypes.byref(p), max(int(nbytes), 8)) == 0
        self._owned.append(p)
        return p

    def copy_in(self, p, a):
        """Host array -> device buffer (blocking)."""
        a = np.ascontiguousarray(a)
        assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, H2D) == 0

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.malloc(a.nbytes)
        self.copy_in(p, a)
        return p

    def poison(self, p, ndoubles):
        """Fill ndoubles float64 words of p with the NaN pattern (blocking)."""
        self.copy_in(p, np.full(int(ndoubles), POISON, dtype=np.uint64))

    def download(self, p, a, sync=True):
        """Device buffer -> host array a. sync=False leaves the waiting to the
        caller (a stream it synchronised itself)."""
        if sync:
            assert self.rt.hipDeviceSynchronize() == 0
        assert self.rt.hipMemcpy(a.ctypes.data, p, a.nbytes, D2H) == 0
        return a

    def free_all(self):
        assert self.rt.hipDeviceSynchronize() == 0
        for p in self._owned:
            self.rt.hipFree(p)
        self._owned = []

    # ---- streams --------------------------------------------------------------
    def stream_create(self):
        s = ctypes.c_void_p()
        assert self.rt.hipStreamCreate(ctypes.byref(s)) == 0
        assert s.value
        return s

    def stream_synchronize(self, s):
        assert self.rt.hipStreamSynchronize(s) == 0

    def stream_destroy(self, s):
        assert self.rt.hipStreamDestroy(s) == 0


def poisoned(a):
    """Count of float64 words of a that still hold the poison pattern."""
    return int(np.count_nonzero(a.view(np.uint64) == POISON))
