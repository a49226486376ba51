"""The WARP rule's CPU spec (tests/c/warp_spec.c), compiled on first use and
linked with the oracle library; shared by test_warp_cpu.py and
test_gpu_warp.py.  One rule, two instances: the reference's fp64 arithmetic
and the project's fp32 arithmetic spec."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import oracle as orc
from tests.conftest import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "c", "warp_spec.c")
_lib = None


def lib():
    global _lib
    if _lib is None:
        orc.lib()   # builds / loads oracle/build/liboracle.so
        odir = os.path.join(ROOT, "oracle", "build")
        tmp = tempfile.mkdtemp(prefix="warp_spec_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libwarp_spec.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-fPIC", "-ffp-contract=off", "-Wall", "-shared",
                        "-I" + os.path.join(ROOT, "oracle"), "-o", so, SRC, "-L" + odir, "-loracle",
                        "-Wl,-rpath," + odir, "-lm"], check=True)
        L = C.CDLL(so)
        u64, P = C.c_uint64, C.c_void_p
        for f in (L.warp_spec_f64, L.warp_spec_f32):
            f.restype = C.c_int
            f.argtypes = [P, P, C.c_int, C.c_double, u64, u64, u64, u64, P, P, P]
        _lib = L
    return _lib


def graph(fname):
    """WARP's graph: directed, negatives uniform ("no_degrees")."""
    return orc.Graph.from_file(os.path.join(GOLDEN, fname), 0, "out_degrees", "no_degrees")


def padded(T, dim):
    dpad = (dim + 3) // 4 * 4
    out = np.zeros((T.shape[0], dpad), np.float32)
    out[:, :dim] = T
    return out


def run(g, T, alpha0, total, begin, end, seed):
    """Samples [begin, end) on T in place (float64 [V][dim], or float32
    [V][dpad]).  Returns (trials per sample, min |f - 1|, trials, updated,
    skipped)."""
    assert T.flags.c_contiguous and T.shape[0] == g.V
    fn = {np.dtype(np.float64): lib().warp_spec_f64, np.dtype(np.float32): lib().warp_spec_f32}[T.dtype]
    nt = np.zeros(end - begin, np.int32)
    margin = C.c_double()
    counts = np.zeros(2, np.uint64)
    skipped = fn(g.ref, orc.ptr(T), T.shape[1], alpha0, total, begin, end, seed, orc.ptr(nt), C.byref(margin),
                 orc.ptr(counts))
    return nt, margin.value, int(counts[0]), int(counts[1]), skipped


def lcg_table(V, dim):
    """The fixtures' starting table: a fixed LCG, U(-0.5, 0.5), row-major."""
    x = 0x243F6A8885A308D3
    out = np.zeros(V * dim)
    for k in range(V * dim):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out[k] = (x >> 11) * 2.0 ** -53 - 0.5
    return out.reshape(V, dim)


def exhaustion_table(V, dim, v, i):
    """T[v] = T[i] = 1, every other row 0: every j outside {v, i} has f = dim >= 1."""
    T = np.zeros((V, dim))
    T[v] = 1.0
    T[i] = 1.0
    return T
