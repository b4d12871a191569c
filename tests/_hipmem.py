"""Device memory for GPU tests on the HIP runtime the library already loaded (no torch in the process: torch bundles its own
HIP runtime, and two runtimes in one process do not share the device)."""
import ctypes as C

import numpy as np


class Hip:
    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), max(int(nbytes), 8)) == 0
        self.bufs.append(p)
        return p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        if arr.nbytes:
            assert self.lib.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0      # hipMemcpyHostToDevice
        return p

    def download(self, ptr, shape, dtype):
        out = np.zeros(shape, dtype=dtype)
        if out.nbytes:
            assert self.lib.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0    # hipMemcpyDeviceToHost
        return out

    def free_all(self):
        for p in self.bufs:
            self.lib.hipFree(p)
        self.bufs = []
