"""The build-and-load step every ctypes wrapper of a CPU oracle shares -- TEST INFRASTRUCTURE.

load = Loader(directory, "libNAME.so", sources, declare): load.build() runs `make -C directory` when the library is missing or
older than one of `sources` (paths relative to the directory: every file its Makefile names as a dependency); load.lib() builds,
opens the library once, hands it to declare(L) to set restype / argtypes, and returns it from then on."""
import ctypes as C
import os
import subprocess


class Loader:
    def __init__(self, here, name, srcs, declare):
        self.here, self.so, self.srcs, self.declare = here, os.path.join(here, name), tuple(srcs), declare
        self._lib = None

    def build(self, force=False):
        so = self.so
        if force or not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(os.path.join(self.here, s)) for s in self.srcs):
            subprocess.check_call(["make", "-C", self.here, "-s"])
        return so

    def lib(self):
        if self._lib is None:
            L = C.CDLL(self.build())
            self.declare(L)
            self._lib = L
        return self._lib
