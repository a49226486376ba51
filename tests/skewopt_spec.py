"""The Skew-OPT rule's CPU spec (tests/c/skewopt_spec.c), compiled on first use
and linked with the oracle library; shared by test_skewopt_cpu.py and
test_gpu_skewopt.py.  One rule, two instances: the reference's fp64 arithmetic
and the project's fp32 arithmetic spec."""
import atexit
import collections
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import oracle as orc
from tests.conftest import GOLDEN, ROOT
from tests.warp_spec import lcg_table, padded  # noqa: F401  (the fixtures' starting table)

SRC = os.path.join(ROOT, "tests", "c", "skewopt_spec.c")
NEG = 16
_lib = None

# rec: [n][18] ids {v, i, j_0..j_15}; trace: [n][16] -1 gated / not run, else the
# sigmoid code; kind: [n][16] 0 gated / not run, 1 clamped, 2 interior; gmin: min |g|
Run = collections.namedtuple("Run", "rec trace kind gmin passed updated skipped")


def lib():
    global _lib
    if _lib is None:
        orc.lib()   # builds / loads oracle/build/liboracle.so
        odir = os.path.join(ROOT, "oracle", "build")
        tmp = tempfile.mkdtemp(prefix="skewopt_spec_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libskewopt_spec.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-fPIC", "-ffp-contract=off", "-Wall", "-shared",
                        "-I" + os.path.join(ROOT, "oracle"), "-o", so, SRC, "-L" + odir, "-loracle",
                        "-Wl,-rpath," + odir, "-lm"], check=True)
        L = C.CDLL(so)
        u64, P, dbl = C.c_uint64, C.c_void_p, C.c_double
        for f in (L.skewopt_spec_f64, L.skewopt_spec_f32):
            f.restype = C.c_int
            f.argtypes = [P, P, C.c_int, dbl, dbl, dbl, C.c_int, u64, u64, u64, u64, P, P, P, P, P, C.c_int64, P]
        _lib = L
    return _lib


def graph(fname):
    """Skew-OPT's graph: directed, negatives uniform ("no_degrees")."""
    return orc.Graph.from_file(os.path.join(GOLDEN, fname), 0, "out_degrees", "no_degrees")


def run(g, T, alpha0, xi, omega, eta, total, begin, end, seed, stop=-1):
    """Samples [begin, end) on T in place (float64 [V][dim], float32 [V][dpad], or
    None: the draws only).  Returns Run.  stop >= 0: the run ends at its negative
    number `stop` before that negative's gate acts, T as the negative found it;
    returns that negative's g instead."""
    n = end - begin
    if T is None:
        fn, d = lib().skewopt_spec_f64, 0
    else:
        assert T.flags.c_contiguous and T.shape[0] == g.V
        fn = {np.dtype(np.float64): lib().skewopt_spec_f64, np.dtype(np.float32): lib().skewopt_spec_f32}[T.dtype]
        d = T.shape[1]
    rec = np.zeros((n, 2 + NEG), np.int32)
    trace = np.zeros((n, NEG), np.int16)
    kind = np.zeros((n, NEG), np.uint8)
    gmin, gstop = C.c_double(), C.c_double()
    counts = np.zeros(2, np.uint64)
    skipped = fn(g.ref, None if T is None else orc.ptr(T), d, alpha0, xi, omega, eta, total, begin, end, seed,
                 orc.ptr(rec), orc.ptr(trace), orc.ptr(kind), C.byref(gmin), orc.ptr(counts), stop, C.byref(gstop))
    if stop >= 0:
        return gstop.value
    return Run(rec, trace, kind, gmin.value, int(counts[0]), int(counts[1]), skipped)


def distinct(rec):
    """Per record: its 18 ids are pairwise distinct (the kernel's fast path)."""
    return np.array([len(set(r.tolist())) == len(r) for r in rec])


def gated_table(V, dim, v, i, c):
    """Rows v and i the constant c, every other row zero: f = dim c^2 at every
    negative outside {v, i}."""
    T = np.zeros((V, dim))
    T[v] = c
    T[i] = c
    return T


def gzero_table(V, dim, v, i, xi):
    """Row v one at element 0, row i xi at element 0, every other row zero:
    f == xi exactly at every negative outside {v, i}, so g == 0."""
    T = np.zeros((V, dim))
    T[v, 0] = 1.0
    T[i, 0] = xi
    return T


def gzero_case():
    """(graph, dim, sample, ids, xi, omega, alpha, seed): a bip.txt sample whose
    negatives avoid v and i, for gzero_table with xi = 0.75 (exact in fp32) and
    the rate 2^-20, at which the decays round to nothing on 1 and 0.75."""
    g = graph("bip.txt")
    seed = 20251015
    rec = run(g, None, 0.025, 0.75, 0.5, 3, TOTAL, 1000, 1200, seed).rec
    for k, r in enumerate(rec):
        if r[1] >= 0 and r[0] != r[1] and r[0] not in r[2:] and r[1] not in r[2:]:
            return g, 8, 1000 + k, r, 0.75, 0.5, 2.0 ** -20, seed
    raise AssertionError("no such sample")


# ---------------------------------------------------------------- the committed reference runs
TOTAL = 10 ** 9   # single-sample trials: alpha stays alpha0


def gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def tags(z):
    return [str(t) for t in z["tags"]]


class Trials:
    """One tag of updates_skewopt.npz: the graph, the parameters and the trial table."""

    def __init__(self, z, tag):
        self.z, self.tag = z, tag
        self.dim, self.eta, self.seed, self.first, self.n = (int(x) for x in z["meta_" + tag])
        self.alpha, self.xi, self.omega, self.c = (float(x) for x in z["meta_" + tag + "_f"])
        self.gfile = str(z["meta_" + tag + "_file"])
        self.g = graph(self.gfile)

    def trial(self, t):
        """(sample, all-gated flag, up, ids[18], pass bits[16], start table, expected table)"""
        s, gated, up = (int(x) for x in self.z[self.tag + "_trial"][t])
        ids = self.z[self.tag + "_ids"][t]
        T0 = gated_table(self.g.V, self.dim, ids[0], ids[1], self.c) if gated else lcg_table(self.g.V, self.dim)
        want = T0.copy()
        for k in range(2 + NEG):
            want[ids[k]] = self.z[self.tag + "_rows"][t][k]
        return s, gated, up, ids, self.z[self.tag + "_pass"][t], T0, want

    def run(self, T, s):
        return run(self.g, T, self.alpha, self.xi, self.omega, self.eta, TOTAL, s, s + 1, self.seed)


def all_trials():
    z = gold("updates_skewopt")
    for tag in tags(z):
        tr = Trials(z, tag)
        for t in range(tr.n):
            yield tr, t


_left_out = None


def left_out():
    """The (tag, t) trials whose fp32 decision trace differs from the fp64 one
    (a gate, clamp or sigmoid bucket decided by rounding): they are not held to
    the reference's table.  Computed once."""
    global _left_out
    if _left_out is None:
        out = set()
        for tr, t in all_trials():
            s, _g, _up, _ids, _p, T0, _want = tr.trial(t)
            a = tr.run(T0.copy(), s)
            b = tr.run(padded(T0.astype(np.float32), tr.dim), s)
            if not (np.array_equal(a.trace, b.trace) and np.array_equal(a.kind, b.kind)):
                out.add((tr.tag, t))
        _left_out = out
    return _left_out


# ---------------------------------------------------------------- scatter quality (bip.txt)
AUC_SAMPLES, AUC_DIM = 200000, 32
AUC_SEEDS = (20251015, 20251016, 20251017)


def glibc_table(V, dim):
    """SPR::Init (src/model/SkewOPT.cpp:45-50): (rand() / RAND_MAX - 0.5) / dim + 0.01, row-major, as fp32."""
    r = orc.glibc_rand(V * dim).astype(np.float64).reshape(V, dim)
    return ((r / 2147483647.0 - 0.5) / dim + 0.01).astype(np.float32)
