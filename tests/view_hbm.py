"""Device buffers for the tracking-view tests: allocate, fill, read back and free through the HIP runtime the library itself is linked
to (tests/color_frames.py: Hbm says why not through torch)."""
import ctypes as C

import numpy as np


class HbmOut:
    def __init__(self):
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so.7")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipDeviceSynchronize.argtypes = []
        self.hip = hip
        self.bufs = []

    def alloc(self, nbytes, fill=0xA5):
        """-> device address of nbytes bytes, every byte `fill`"""
        dev = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(dev), C.c_size_t(nbytes)) == 0
        self.bufs.append(dev)
        host = np.full(nbytes, fill, np.uint8)
        assert self.hip.hipMemcpy(dev, C.c_void_p(host.ctypes.data), C.c_size_t(nbytes), 1) == 0
        return dev.value

    def read(self, dev, nbytes):
        """nbytes bytes at device address `dev` -> uint8 array (after everything on the device has finished)"""
        assert self.hip.hipDeviceSynchronize() == 0
        host = np.empty(nbytes, np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(dev), C.c_size_t(nbytes), 2) == 0
        return host

    def close(self):
        self.hip.hipDeviceSynchronize()
        for d in self.bufs:
            assert self.hip.hipFree(d) == 0
        self.bufs = []
