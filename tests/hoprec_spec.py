"""The HOP-REC rule's CPU spec (tests/c/hoprec_spec.c), compiled on first use
and linked with the oracle library; shared by test_hoprec_cpu.py and
test_gpu_hoprec.py.  One rule, two instances: the reference's fp64 arithmetic
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

SRC = os.path.join(ROOT, "tests", "c", "hoprec_spec.c")
NEG = 5
_lib = None

Run = collections.namedtuple("Run", "rec slots passed margin tested npassed skipped")


def lib():
    global _lib
    if _lib is None:
        orc.lib()   # builds / loads oracle/build/liboracle.so
        odir = os.path.join(ROOT, "oracle", "build")
        tmp = tempfile.mkdtemp(prefix="hoprec_spec_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libhoprec_spec.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-fPIC", "-ffp-contract=off", "-Wall", "-shared",
                        "-I" + os.path.join(ROOT, "oracle"), "-o", so, SRC, "-L" + odir, "-loracle",
                        "-Wl,-rpath," + odir, "-lm"], check=True)
        L = C.CDLL(so)
        u64, P = C.c_uint64, C.c_void_p
        for f in (L.hoprec_spec_f64, L.hoprec_spec_f32):
            f.restype = C.c_int
            f.argtypes = [P, P, P, C.c_int, C.c_int, C.c_double, u64, u64, u64, u64, P, P, P, P, P, C.c_int64, P]
        _lib = L
    return _lib


def width(steps):
    return (1 + (1 + NEG) * steps + 3) // 4 * 4


def graph(fname):
    """HOP-REC's graph: undirected, negatives uniform ("no_degrees")."""
    return orc.Graph.from_file(os.path.join(GOLDEN, fname), 1, "out_degrees", "no_degrees")


def load_fields(g, fname):
    """proNet::LoadFieldMeta (src/proNet.cpp:330-408) in Python: (field[V] int32, fields).
    A field's id is its order of first appearance; unnamed vertices keep 0."""
    ids = {n: k for k, n in enumerate(g.names)}
    meta, field = {}, np.zeros(g.V, np.int32)
    with open(os.path.join(GOLDEN, fname)) as f:
        tok = f.read().split()
    for name, m in zip(tok[0::2], tok[1::2]):
        fid = meta.setdefault(m, len(meta))
        if name in ids:
            field[ids[name]] = fid
    return field, len(meta)


def run(g, field, T, steps, alpha0, total, begin, end, seed, stop=-1):
    """Samples [begin, end) on T in place (float64 [V][dim], float32 [V][dpad], or
    None: the draws only).  Returns Run(records, slots per sample, gate pass bits
    [n][steps][5], min fp64 |f - margin_w|, gates tested, gates passed, skipped).
    stop >= 0: the run ends at its gate number `stop` before that gate acts, T as
    the gate found it; returns that gate's f instead."""
    n = end - begin
    field = np.ascontiguousarray(field, np.int32)
    assert field.shape == (g.V,)
    if T is None:
        fn, d = lib().hoprec_spec_f64, 0
    else:
        assert T.flags.c_contiguous and T.shape[0] == g.V
        fn = {np.dtype(np.float64): lib().hoprec_spec_f64, np.dtype(np.float32): lib().hoprec_spec_f32}[T.dtype]
        d = T.shape[1]
    rec = np.zeros((n, width(steps)), np.int32)
    slots = np.zeros(n, np.uint32)
    passed = np.zeros((n, steps, NEG), np.uint8)
    margin, fstop = C.c_double(), C.c_double()
    counts = np.zeros(2, np.uint64)
    skipped = fn(g.ref, orc.ptr(field), None if T is None else orc.ptr(T), d, steps, alpha0, total, begin, end, seed,
                 orc.ptr(rec), orc.ptr(slots), orc.ptr(passed), C.byref(margin), orc.ptr(counts), stop,
                 C.byref(fstop))
    if stop >= 0:
        return fstop.value
    return Run(rec, slots, passed, margin.value, int(counts[0]), int(counts[1]), skipped)


def closed_table(V, dim, rec, steps):
    """Rows v and every i_w all ones, every other row zero: every gate of the
    sample has f = dim > margin (its negatives touch neither v nor an i_w)."""
    T = np.zeros((V, dim))
    T[rec[0]] = 1.0
    for w in range(steps):
        T[rec[1 + (1 + NEG) * w]] = 1.0
    return T


# ---------------------------------------------------------------- the committed reference runs
TOTAL = 10 ** 9   # single-sample trials: alpha stays alpha0
TAGS = ("bip16", "bip64", "pl3")


def gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


class Trials:
    """One tag of updates_hoprec.npz: the graph, the fields and the trial table."""

    def __init__(self, z, tag):
        self.z, self.tag = z, tag
        self.dim, self.steps, self.seed, self.first, self.n = (int(x) for x in z["meta_" + tag])
        self.alpha = float(z["meta_" + tag + "_f"][0])
        self.gfile, self.ffile = (str(x) for x in z["meta_" + tag + "_files"])
        self.g = graph(self.gfile)
        self.field, self.nfields = load_fields(self.g, self.ffile)
        self.nw = 1 + 6 * self.steps

    def trial(self, t):
        """(sample, slots, kind, rejected, record, pass bits, start table, expected table)"""
        s, slots, kind, rej = (int(x) for x in self.z[self.tag + "_trial"][t])
        rec = self.z[self.tag + "_rec"][t]
        T0 = closed_table(self.g.V, self.dim, rec, self.steps) if kind else lcg_table(self.g.V, self.dim)
        want = T0.copy()
        for k in range(self.nw):
            want[rec[k]] = self.z[self.tag + "_rows"][t][k]
        return s, slots, kind, rej, rec, self.z[self.tag + "_pass"][t], T0, want

    def run(self, T, s):
        return run(self.g, self.field, T, self.steps, self.alpha, TOTAL, s, s + 1, self.seed)


# ---------------------------------------------------------------- scatter quality (bip.txt)
AUC_SAMPLES, AUC_DIM, AUC_STEPS = 200000, 32, 5
AUC_SEEDS = (20251015, 20251016, 20251017)
# the fp32 spec's AUC after AUC_SAMPLES samples from HBPR::Init's table at the three
# seeds (test_hoprec_cpu.py recomputes them); the GPU scatter test's bar comes from these
SPEC_AUC = (0.9115, 0.9065, 0.9105)


def glibc_table(V, dim):
    """HBPR::Init (src/model/HBPR.cpp:50-54): (rand() / RAND_MAX - 0.5) / dim, row-major, as fp32."""
    r = orc.glibc_rand(V * dim).astype(np.float64).reshape(V, dim)
    return ((r / 2147483647.0 - 0.5) / dim).astype(np.float32)


def auc(g, field, T, seed=5):
    """Every user -> item training positive against one uniform item-field negative."""
    u = np.repeat(np.arange(g.V), np.diff(g.offsets))
    i = g.targets[:g.E]
    keep = (field[u] == 0) & (field[i] != 0)
    u, i = u[keep], i[keep]
    items = np.nonzero(field != 0)[0]
    j = items[np.random.default_rng(seed).integers(0, len(items), len(u))]
    T = T.astype(np.float64)
    x = (T[u] * (T[i] - T[j])).sum(1)
    return float((x > 0).mean() + 0.5 * (x == 0).mean())
