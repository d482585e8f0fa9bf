"""ctypes driver of tests/cpp/pool_sim.cpp: the product's clip-pool policy (whitebox_amd/csrc/wbx_pool.h) compiled with
plain g++ and run on the CPU, its memory a callback that hands out none.  TEST INFRASTRUCTURE — nothing here is shipped."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import List, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pool_sim.cpp")
MAIN = os.path.join(ROOT, "tests", "cpp", "pool_main.cpp")
HDR = os.path.join(ROOT, "whitebox_amd", "csrc", "wbx_pool.h")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
FLAGS = ["-std=c++17", "-Wall", "-Wextra"]

_lib = None


def build_lib() -> str:
    """libwbxpoolsim.so, rebuilt when a source is newer (to a name of its own, then renamed: pytest-xdist workers build
    side by side and must never load half a file)"""
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "libwbxpoolsim.so")
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in (SRC, HDR)):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", *FLAGS, "-O2", "-shared", "-fPIC", SRC, "-o", tmp])
        os.replace(tmp, out)
    return out


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        L = C.CDLL(build_lib())
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        L.psim_create.restype = vp
        L.psim_create.argtypes = []
        for name, res, args in (
                ("psim_destroy", None, [vp]), ("psim_set_limit", None, [vp, u64]), ("psim_set_driver_fails", None, [vp, C.c_int]),
                ("psim_extent", None, [u64, u32, C.c_int, C.POINTER(u64), C.POINTER(u64)]),
                ("psim_take", C.c_int, [vp, u64, u64, C.c_int, C.POINTER(u32), C.POINTER(C.c_int32), C.POINTER(u64)]),
                ("psim_give", C.c_int, [vp, u32]),
                ("psim_stats", None, [vp, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
                ("psim_dump", C.c_int, [vp, u32, C.POINTER(u64), C.POINTER(u64), u32])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def extent(nbytes: int, placed: int, jitter: bool = True) -> Tuple[int, int]:
    body, gap = C.c_uint64(), C.c_uint64()
    lib().psim_extent(nbytes, placed, int(jitter), C.byref(body), C.byref(gap))
    return body.value, gap.value


class PoolSim:
    def __init__(self):
        self.L = lib()
        self.h = C.c_void_p(self.L.psim_create())

    def close(self):
        if self.h:
            self.L.psim_destroy(self.h)
        self.h = None

    def set_limit(self, limit: int): self.L.psim_set_limit(self.h, limit)
    def set_driver_fails(self, fails: bool): self.L.psim_set_driver_fails(self.h, int(fails))

    def take(self, need: int, own_bytes: int, use_slabs: bool = True):
        """-> (where, id or None, slab index, offset)"""
        i, slab, off = C.c_uint32(), C.c_int32(), C.c_uint64()
        where = self.L.psim_take(self.h, need, own_bytes, int(use_slabs), C.byref(i), C.byref(slab), C.byref(off))
        return where, (i.value if where in (0, 1) else None), slab.value, off.value

    def give(self, i: int):
        assert self.L.psim_give(self.h, i) == 0, f"no live extent {i}"

    def stats(self) -> Tuple[int, int, int]:
        n, res, live, calls = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.L.psim_stats(self.h, C.byref(n), C.byref(res), C.byref(live), C.byref(calls))
        return n.value, res.value, live.value

    def dump(self, slab: int):
        """-> (size, used, live, live_bytes, [(offset, bytes) of every hole])"""
        info = (C.c_uint64 * 4)()
        n = self.L.psim_dump(self.h, slab, info, None, 0)
        assert n >= 0, f"no slab {slab}"
        buf = (C.c_uint64 * (2 * max(n, 1)))()
        assert self.L.psim_dump(self.h, slab, info, buf, n) == n
        holes: List[Tuple[int, int]] = [(buf[2 * k], buf[2 * k + 1]) for k in range(n)]
        return info[0], info[1], info[2], info[3], holes
