"""The CSE rule's CPU spec (tests/c/cse_spec.c: nemf and nerank), compiled on
first use and linked with the oracle library; shared by test_cse_cpu.py and
test_gpu_cse.py.  One rule, two instances: the reference's fp64 arithmetic and
the project's fp32 arithmetic spec."""
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
from tests.hoprec_spec import load_fields  # noqa: F401
from tests.warp_spec import lcg_table, padded  # noqa: F401

SRC = os.path.join(ROOT, "tests", "c", "cse_spec.c")
NEG, RANK_NEG = 5, 16
NEMF, NERANK = 0, 1
WU, WI, CU, CI = 0, 1, 2, 3
_lib = None

Run = collections.namedtuple("Run", "rec slots used passed margin tested updated skipped")


def lib():
    global _lib
    if _lib is None:
        orc.lib()   # builds / loads oracle/build/liboracle.so
        odir = os.path.join(ROOT, "oracle", "build")
        tmp = tempfile.mkdtemp(prefix="cse_spec_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libcse_spec.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-fPIC", "-ffp-contract=off", "-Wall", "-shared",
                        "-I" + os.path.join(ROOT, "oracle"), "-o", so, SRC, "-L" + odir, "-loracle",
                        "-Wl,-rpath," + odir, "-lm"], check=True)
        L = C.CDLL(so)
        u64, P = C.c_uint64, C.c_void_p
        for f in (L.cse_spec_f64, L.cse_spec_f32):
            f.restype = C.c_int
            f.argtypes = [P, P, P, P, P, P, C.c_int, C.c_int, C.c_int, C.c_double, u64, u64, u64, u64, P, P, P, P, P,
                          P, C.c_int64, P]
        _lib = L
    return _lib


def dneg(rank):
    return RANK_NEG if rank else NEG


def nwords(steps, rank):
    return 12 * steps + dneg(rank)


def width(steps, rank):
    return (nwords(steps, rank) + 3) // 4 * 4


def table_of_word(k, steps):
    """The table that record word k addresses: v -> WU, c -> WI, pass A's
    contexts -> CI, pass B's -> CU, the direct negatives -> WI."""
    if k < 2:
        return k
    return CI if k < 1 + 6 * steps else CU if k < 12 * steps else WI


def graph(fname):
    """CSE's graph: undirected, sources by out-degree, negatives by degree."""
    return orc.Graph.from_file(os.path.join(GOLDEN, fname), 1, "out_degrees", "degrees")


def run(g, field, T, steps, rank, alpha0, total, begin, end, seed, stop=-1):
    """Samples [begin, end) on T = (WU, WI, CU, CI) in place (four float64 [V][dim]
    or float32 [V][dpad] arrays, or None: the draws only).  Returns Run(records,
    slots drawn, slots the reference consumes, per sample the nerank negative that
    passed (-1 none, nemf 0, -2 no sample), min fp64 |f - 1| over the nerank gates,
    gates tested, nerank updates, skipped).  stop >= 0: the run ends at its nerank
    gate number `stop` before that gate acts; returns that gate's f instead."""
    n = end - begin
    field = np.ascontiguousarray(field, np.int32)
    assert field.shape == (g.V,)
    if T is None:
        fn, d, ptrs = lib().cse_spec_f64, 0, [None] * 4
    else:
        assert len(T) == 4
        for t in T:
            assert t.flags.c_contiguous and t.shape == T[0].shape and t.dtype == T[0].dtype and t.shape[0] == g.V
        fn = {np.dtype(np.float64): lib().cse_spec_f64, np.dtype(np.float32): lib().cse_spec_f32}[T[0].dtype]
        d, ptrs = T[0].shape[1], [orc.ptr(t) for t in T]
    rec = np.zeros((n, width(steps, rank)), np.int32)
    slots, used = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    passed = np.zeros(n, np.int32)
    margin, fstop = C.c_double(), C.c_double()
    counts = np.zeros(2, np.uint64)
    skipped = fn(g.ref, orc.ptr(field), *ptrs, d, steps, rank, alpha0, total, begin, end, seed, orc.ptr(rec),
                 orc.ptr(slots), orc.ptr(used), orc.ptr(passed), C.byref(margin), orc.ptr(counts), stop,
                 C.byref(fstop))
    if stop >= 0:
        return fstop.value
    return Run(rec, slots, used, passed, margin.value, int(counts[0]), int(counts[1]), skipped)


def pad4(T, dim):
    """The four fp32 padded tables of four fp64 ones."""
    return [padded(np.asarray(t).astype(np.float32), dim) for t in T]


# ---------------------------------------------------------------- the committed reference runs
TOTAL = 10 ** 9   # single-sample trials: alpha stays alpha0
TAGS = ("toy5s1", "toy16s2", "bip16s5", "bip64s2", "bip5s1", "pl5s5", "pl64s1")
RANKS = ("nemf", "nerank")


def gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def start_tables(V, dim, scale):
    """The trials' starting tables: one LCG stream over WU, WI, CU, CI in turn;
    WU and WI times `scale` (nerank: so that f spreads around the margin 1)."""
    T = lcg_table(4 * V, dim).reshape(4, V, dim)
    return [T[0] * scale, T[1] * scale, T[2].copy(), T[3].copy()]


class Trials:
    """One (model, tag) of updates_cse.npz: the graph, the fields and the trial table."""

    def __init__(self, z, rank, tag):
        self.z, self.rank, self.key = z, rank, RANKS[rank] + "_" + tag
        self.dim, self.steps, self.seed, self.first, self.n = (int(x) for x in z["meta_" + self.key])
        self.alpha, self.scale = (float(x) for x in z["meta_" + self.key + "_f"])
        self.gfile, self.ffile = (str(x) for x in z["meta_" + self.key + "_files"])
        self.g = graph(self.gfile)
        self.field, self.nfields = load_fields(self.g, self.ffile)
        self.nw = nwords(self.steps, rank)
        self.start = start_tables(self.g.V, self.dim, self.scale)

    def trial(self, t):
        """(sample, slots the reference consumed, closed, direct negatives drawn, pass
        index, record, start tables, expected tables)"""
        s, slots, closed, nd, pidx = (int(x) for x in self.z[self.key + "_trial"][t])
        rec = self.z[self.key + "_rec"][t]
        T0 = [x.copy() for x in self.start]
        if closed:   # rows WU[v], WI[c] all ones, every other WI row zero: f = dim > 1 at every gate
            T0[WU][rec[0]] = 1.0
            T0[WI][:] = 0.0
            T0[WI][rec[1]] = 1.0
        want = [x.copy() for x in T0]
        rows = self.z[self.key + "_rows"][t]
        for k in range(self.nw):
            if rec[k] >= 0:
                want[table_of_word(k, self.steps)][rec[k]] = rows[k]
        want[CI][rec[0]] = rows[self.nw]
        want[CU][rec[1]] = rows[self.nw + 1]
        return s, slots, closed, nd, pidx, rec, T0, want

    def run(self, T, s):
        return run(self.g, self.field, T, self.steps, self.rank, self.alpha, TOTAL, s, s + 1, self.seed)


def all_trials(z=None):
    z = gold("updates_cse") if z is None else z
    return {(rank, tag): Trials(z, rank, tag) for rank in (NEMF, NERANK) for tag in TAGS}


# ---------------------------------------------------------------- scatter quality (bip.txt)
AUC_SAMPLES, AUC_DIM, AUC_STEPS = 200000, 32, 5
AUC_SEEDS = (20251015, 20251016, 20251017)
# the fp32 spec's AUC after AUC_SAMPLES samples from Init's tables at the three seeds
# (test_cse_cpu.py recomputes them); the GPU scatter test's bar comes from these
SPEC_AUC = {NEMF: (0.8980, 0.9035, 0.9005), NERANK: (0.8215, 0.8250, 0.8200)}


def glibc_tables(V, dim):
    """NEMF::Init (src/model/NEMF.cpp:62-82): WU[v][d] and WI[v][d] drawn in turn from
    one rand() stream, (rand() / RAND_MAX - 0.5) / dim; CU and CI zero.  As fp32."""
    r = orc.glibc_rand(2 * V * dim).astype(np.float64).reshape(V, dim, 2)
    x = ((r / 2147483647.0 - 0.5) / dim).astype(np.float32)
    z = np.zeros((V, dim), np.float32)
    return [np.ascontiguousarray(x[:, :, 0]), np.ascontiguousarray(x[:, :, 1]), z, z.copy()]


def auc(g, field, TU, TI, seed=5):
    """Every user -> item training positive against one uniform item-field negative, scored WU[u] . WI[i]."""
    u = np.repeat(np.arange(g.V), np.diff(g.offsets))
    i = g.targets[:g.E]
    keep = (field[u] == 0) & (field[i] != 0)
    u, i = u[keep], i[keep]
    items = np.nonzero(field != 0)[0]
    j = items[np.random.default_rng(seed).integers(0, len(items), len(u))]
    TU, TI = TU.astype(np.float64), TI.astype(np.float64)
    x = (TU[u] * (TI[i] - TI[j])).sum(1)
    return float((x > 0).mean() + 0.5 * (x == 0).mean())

