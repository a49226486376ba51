"""The sampled-softmax choice (ECO) rule's CPU spec (tests/c/eco_spec.c), compiled on first use
and linked with the oracle library; shared by test_eco_cpu.py and test_gpu_eco.py.  One rule,
two instances: the reference's fp64 arithmetic and the project's fp32 arithmetic spec, whose
exponential is smore_amd/csrc/exp32.h, the header the kernel includes."""
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

SRC = os.path.join(ROOT, "tests", "c", "eco_spec.c")
LISTS = 5
_lib = None

Run = collections.namedtuple("Run", "rec slots clean skipped")


def lib():
    global _lib
    if _lib is None:
        orc.lib()   # builds / loads oracle/build/liboracle.so
        odir = os.path.join(ROOT, "oracle", "build")
        tmp = tempfile.mkdtemp(prefix="eco_spec_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libeco_spec.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-fPIC", "-ffp-contract=off", "-Wall", "-shared",
                        "-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(ROOT, "smore_amd", "csrc"), "-o", so, SRC,
                        "-L" + odir, "-loracle", "-Wl,-rpath," + odir, "-lm"], check=True)
        L = C.CDLL(so)
        u64, P = C.c_uint64, C.c_void_p
        for f in (L.eco_spec_f64, L.eco_spec_f32):
            f.restype = C.c_int
            f.argtypes = [P, P, P, C.c_int, C.c_int, C.c_double, C.c_double, u64, u64, u64, u64, P, P, P]
        L.eco_loss.restype = C.c_double
        L.eco_loss.argtypes = [P, C.c_int, C.c_int, P]
        L.eco_exp32_worst.restype = C.c_double
        L.eco_exp32_worst.argtypes = [C.c_double, C.c_double, C.c_int64, C.POINTER(C.c_double)]
        L.eco_exp32.restype = C.c_float
        L.eco_exp32.argtypes = [C.c_float]
        _lib = L
    return _lib


def nwords(K):
    return 1 + LISTS * (2 + K)


def width(K):
    return (nwords(K) + 3) // 4 * 4


def graph(fname, undirected=1):
    """ECO's graph: sources by out-degree, negatives uniform (ECO() sets no_degrees)."""
    return orc.Graph.from_file(os.path.join(GOLDEN, fname), undirected, "out_degrees", "no_degrees")


def run(g, field, T, K, alpha0, reg, total, begin, end, seed):
    """Samples [begin, end) on T in place (float64 [V][dim], float32 [V][dpad], or None: the
    draws only).  Returns Run(records, slots drawn, clean (1 clean, 0 ordered, -1 skipped),
    skipped)."""
    n = end - begin
    field = np.ascontiguousarray(field, np.int32)
    assert field.shape == (g.V,)
    if T is None:
        fn, d, p = lib().eco_spec_f64, 0, None
    else:
        assert T.flags.c_contiguous and T.shape[0] == g.V
        fn = {np.dtype(np.float64): lib().eco_spec_f64, np.dtype(np.float32): lib().eco_spec_f32}[T.dtype]
        d, p = T.shape[1], orc.ptr(T)
    rec = np.zeros((n, width(K)), np.int32)
    slots = np.zeros(n, np.uint32)
    clean = np.zeros(n, np.int32)
    skipped = fn(g.ref, orc.ptr(field), p, d, K, alpha0, reg, total, begin, end, seed, orc.ptr(rec), orc.ptr(slots),
                 orc.ptr(clean))
    return Run(rec, slots, clean, skipped)


def loss(T, K, rec):
    """The rule's objective: the mean over the lists of the records of log(sum) - log(2 e1 +
    e2), in fp64 on table T."""
    T = np.ascontiguousarray(T[:, :], np.float64)
    rec = np.ascontiguousarray(rec, np.int32)
    keep = [r for r in rec if r[0] >= 0]
    return float(np.mean([lib().eco_loss(orc.ptr(T), T.shape[1], K, orc.ptr(r)) for r in keep])) / LISTS


def exp32(x):
    return float(lib().eco_exp32(float(x)))


def exp32_worst(lo, hi, n):
    """(worst relative error of exp32 against double exp over n evenly spaced arguments, where)"""
    at = C.c_double()
    return float(lib().eco_exp32_worst(lo, hi, n, C.byref(at))), at.value


def save_lines(g, W, fmt="%g"):
    """ECO::SaveWeights (src/model/ECO.cpp:19-39) on an fp64 table, as bytes."""
    out = ["%d %d\n" % (g.V, W.shape[1])]
    for v in range(g.V):
        out.append(g.names[v] + "".join(" " + fmt % x for x in W[v]) + "\n")
    return "".join(out).encode()


# ---------------------------------------------------------------- the committed reference runs
TOTAL = 10 ** 9   # single-sample trials: alpha stays alpha0
TAGS = ("toy5k1", "toy16k5", "bip16k5", "bip64k20", "bip5k1", "pl5k5", "pl64k5", "toyd5k5")


def gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def start_table(V, dim):
    """The trials' starting w_vertex: the first V rows of the `updates` mode's LCG stream."""
    return np.ascontiguousarray(lcg_table(V, dim))


class Trials:
    """One tag of updates_eco.npz: the graph, the fields and the trial table."""

    def __init__(self, z, tag):
        self.z, self.key = z, tag
        self.dim, self.K, self.undirected, self.seed, self.first, self.n = (int(x) for x in z["meta_" + tag])
        self.alpha, self.reg = (float(x) for x in z["meta_" + tag + "_f"])
        self.gfile, self.ffile = (str(x) for x in z["meta_" + tag + "_files"])
        self.g = graph(self.gfile, self.undirected)
        self.field, self.nfields = load_fields(self.g, self.ffile)
        self.nw = nwords(self.K)
        self.start = start_table(self.g.V, self.dim)

    def trial(self, t):
        """(sample, slots consumed, record, start table, expected table)"""
        s, slots = (int(x) for x in self.z[self.key + "_trial"][t])
        rec = self.z[self.key + "_rec"][t]
        assert bool(self.z[self.key + "_others_unchanged"][t])
        want = self.start.copy()
        rows = self.z[self.key + "_rows"][t]
        for k in range(self.nw):
            if rec[k] >= 0:
                want[rec[k]] = rows[k]
        return s, slots, rec, self.start.copy(), want

    def run(self, T, s):
        return run(self.g, self.field, T, self.K, self.alpha, self.reg, TOTAL, s, s + 1, self.seed)


def all_trials(z=None):
    z = gold("updates_eco") if z is None else z
    return {tag: Trials(z, tag) for tag in TAGS}


def lists_of(rec, K):
    """[(c1, c2, [negatives])] of a record."""
    return [(int(rec[1 + b * (2 + K)]), int(rec[2 + b * (2 + K)]), [int(x) for x in rec[3 + b * (2 + K):3 + b * (2 + K) + K]])
            for b in range(LISTS)]


def is_clean(rec, K):
    ids = [int(x) for x in rec[:nwords(K)]]
    return len(set(ids)) == len(ids)


def special_cases(rec, K):
    """The coincidences a record holds: a subset of {"skip", "clean", "neg=v", "c2=v", "c1=c2",
    "dup-neg", "shared"}."""
    if rec[0] < 0:
        return {"skip"}
    out, v, seen = set(), int(rec[0]), set()
    if is_clean(rec, K):
        out.add("clean")
    for c1, c2, neg in lists_of(rec, K):
        if v in neg:
            out.add("neg=v")
        if c2 == v:
            out.add("c2=v")
        if c1 == c2:
            out.add("c1=c2")
        if len(set(neg)) < len(neg):
            out.add("dup-neg")
        if seen & {c1, c2, *neg}:
            out.add("shared")
        seen |= {c1, c2, *neg}
    return out


# ---------------------------------------------------------------- whole run
E2E = ("e2e_eco_bip", "bip.txt", "bip_field.txt")
# max |fp32 spec - reference| over the committed 10^6-sample run (test_eco_cpu.py measures it):
# 1.8e-5, at most 1e-4, so the class and the CLI in serial are held to the reference's own W
# and saved file at E2E_GAP_BOUND
E2E_GAP_BOUND = 1e-4


def glibc_tables(V, dim):
    """ECO::Init: w_vertex[v][d] then w_ignore[v][d] from one rand() stream, rand() / RAND_MAX -
    0.5, not divided by dim.  As fp64."""
    r = orc.glibc_rand(2 * V * dim).astype(np.float64).reshape(V, dim, 2)
    x = r / 2147483647.0 - 0.5
    return np.ascontiguousarray(x[:, :, 0]), np.ascontiguousarray(x[:, :, 1])


# ---------------------------------------------------------------- scatter quality (bip.txt)
Q_SAMPLES, Q_DIM, Q_K, Q_ALPHA, Q_REG = 200000, 32, 5, 0.025, 0.01
Q_SEEDS = (20251015, 20251016, 20251017)
Q_EVAL_SEED, Q_EVAL = 777, 2000
# the fp32 spec's objective (loss() on Q_EVAL records of seed Q_EVAL_SEED) after Q_SAMPLES samples
# from Init's table at the three seeds, and the untrained table's (test_eco_cpu.py recomputes
# them).  The GPU scatter test's bar comes from these.
Q_SPEC = (-0.3107, -0.3107, -0.3115)
Q_UNTRAINED = 0.9244


def q_bar():
    """The worst spec value plus three times the spread over the seeds."""
    return max(Q_SPEC) + 3 * (max(Q_SPEC) - min(Q_SPEC))


def q_eval_records(g, field):
    return run(g, field, None, Q_K, Q_ALPHA, Q_REG, TOTAL, 0, Q_EVAL, Q_EVAL_SEED).rec


# ---------------------------------------------------------------- the together path under load
LOAD_USERS, LOAD_ITEMS, LOAD_LINES, LOAD_SEED = 4096, 16384, 200000, 11


def load_graph(edges):
    """A generated bipartite graph, loaded undirected: users (field 0) [0, LOAD_USERS), items
    (field 1) after them.  edges = smore_amd.graphgen.bipartite_edges(...)."""
    src, dst, w = edges
    s2, d2, w2 = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([w, w])
    V = LOAD_USERS + LOAD_ITEMS
    return orc.Graph(V, s2, d2, w2, "out_degrees", "no_degrees"), (np.arange(V) >= LOAD_USERS).astype(np.int32), (s2, d2, w2)
