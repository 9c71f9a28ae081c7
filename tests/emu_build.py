"""The build step of the CPU emulation libraries (emu_c, emu_crop_c, emu_resize_c, emu_resize_aa_c, emu_scaled_c).  TEST ONLY."""
import ctypes
import fcntl
import os
import subprocess


def build(so, srcs, opt, extra=()):
    """Compile srcs[0] into the shared library `so` with g++ if it is missing or older than any of srcs (the .cpp and the
    headers it includes).  opt: "-O1" or "-O2"; extra: the library's own flags.  Returns so."""
    def stale():
        return not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)
    if stale():
        # pytest-xdist workers import this together: one of them builds (to a name of its own, renamed when whole),
        # the others wait at the lock and find the library fresh
        with open(so + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                tmp = f"{so}.{os.getpid()}.tmp"
                subprocess.check_call(["g++", opt, "-g", "-std=c++17", "-fPIC", "-shared", "-fno-strict-aliasing", *extra,
                                       "-Wall", "-Wno-unknown-pragmas", "-o", tmp, srcs[0]])
                os.replace(tmp, so)
    return so


HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "zune-jpeg_amd", "csrc")
_LIBS = {}


def load(folder, so, cpp, headers, opt, extra=(), bind=None):
    """The emulation tests/<folder>/<cpp> as a ctypes library, loaded once: built into tests/<folder>/<so> when that is older
    than the .cpp or one of `headers` (names under zune-jpeg_amd/csrc, or paths from tests/); bind(L) declares its functions."""
    if so not in _LIBS:
        srcs = [os.path.join(HERE, folder, cpp)] + [os.path.join(HERE if "/" in h else CSRC, h) for h in headers]
        L = ctypes.CDLL(build(os.path.join(HERE, folder, so), srcs, opt, extra))
        if bind:
            bind(L)
        _LIBS[so] = L
    return _LIBS[so]
