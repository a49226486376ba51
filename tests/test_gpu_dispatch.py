"""Routing of the update-kernel families: a parallel-mode call of exactly ONE
sample is deterministic and must equal the oracle's fp32 spec from the same
tables, so a call that reached the wrong instantiation (another family,
another KMAX bucket and with it another record width, another lane layout)
shows up as a wrong set of updated rows or as wrong values.  Needs an MI355X.

Serial parity (test_gpu_parity.py, test_gpu_go.py, test_gpu_pairs.py,
test_gpu_warp.py) covers every KMAX bucket of the serial path; this file
covers (family, scatter mode, KMAX, lane layout) of the parallel modes.

Every case asserts, for three sample indices:
  * the rows that differ from the initial tables are exactly the oracle's;
  * the values agree within 1e-6 absolute (test_hybrid_single_sample's bound).
"""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import warp_spec as ws
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

SEED = 20251015
ATOL = 1e-6
SAMPLES = (5, 99, 12345)
# (scatter mode, hot threshold): hybrid with every row hot (atomic deltas, the
# hottest write-combined) and with no row hot (plain stores)
MODES = [("atomic", None), ("hogwild", None), ("hybrid", 0.0), ("hybrid", 1e30)]
MODE_IDS = ["atomic", "hogwild", "hybrid-hot", "hybrid-cold"]


@pytest.fixture(scope="module")
def smore():
    import smore_amd
    return smore_amd


_graphs = {}


def oracle_graph(fname, und, go=False, nm="degrees"):
    key = (fname, und, go, nm)
    if key not in _graphs:
        path = os.path.join(GOLDEN, fname)
        _graphs[key] = orc.GoGraph.from_file(path, und) if go else orc.Graph.from_file(path, und, "out_degrees", nm)
    return _graphs[key]


def pronet(smore, fname, und, go=False, nm="degrees"):
    pn = smore.ProNet(0)
    pn.SetNegativeMethod(nm)
    pn.LoadEdgeList(os.path.join(GOLDEN, fname), und)
    if go:
        pn.set_semantics("go")
    return pn


def rand_tables(V, dim, seed):
    rng = np.random.default_rng(seed)
    return [(rng.random((V, dim), dtype=np.float32) - 0.5) for _ in range(2)]


def padded(T, dim):
    out = np.zeros((T.shape[0], (dim + 3) // 4 * 4), np.float32)
    out[:, :dim] = T
    return out


def changed(T, T0):
    return np.flatnonzero((T != T0).any(axis=1))


def check(pn, dim, start, want, what):
    """Tables `start` (as set on the device) against the oracle's `want`
    (padded): the same rows changed, the same values within ATOL."""
    n_changed = 0
    for t, (T0, Tw) in enumerate(zip(start, want)):
        got = pn.get_table(t)
        rows_want = changed(Tw[:, :dim], T0)
        np.testing.assert_array_equal(changed(got, T0), rows_want, err_msg="%s: updated rows of table %d" % (what, t))
        np.testing.assert_allclose(got, Tw[:, :dim], atol=ATOL, rtol=0, err_msg="%s: table %d" % (what, t))
        n_changed += len(rows_want)
    return n_changed


def set_tables(pn, start):
    for t, T0 in enumerate(start):
        pn.set_table(t, T0)


# ---------------------------------------------------------------- C++ edge kernel
# every KMAX bucket (K 5 / 9 / 17 -> 5 / 10 / 20) under every mode setting, the
# dims (8: G = 2, 64: G = 16, 300: G = 64 with two registers per lane)
# rotating over the pairs; LINE-1 (the shared table) and BPR under every mode
def _edge_cases():
    dims, out = (8, 64, 300), []
    for i, K in enumerate((5, 9, 17)):
        for j in range(len(MODES)):
            out.append(("line2", K, dims[(i + j) % 3], j))
    for j in range(len(MODES)):
        out.append(("line1", 5, dims[(j + 1) % 3], j))
        out.append(("bpr", 5, dims[j % 3], j))
    return out


@pytest.mark.parametrize("model,K,dim,mi", _edge_cases(),
                         ids=["%s-K%d-d%d-%s" % (m, K, d, MODE_IDS[j]) for m, K, d, j in _edge_cases()])
def test_cpp_edge_routing(smore, model, K, dim, mi):
    mode, tau = MODES[mi]
    fname, und, nm = ("bip.txt", 0, "no_degrees") if model == "bpr" else ("pl100w.txt", 1, "degrees")
    g, pn = oracle_graph(fname, und, nm=nm), pronet(smore, fname, und, nm=nm)
    ntab = 2 if model == "line2" else 1
    start = rand_tables(g.V, dim, dim * 7 + K)[:ntab]
    pn.alloc_tables(dim, ntab)
    if tau is not None:
        pn.set_hot_threshold(tau)
    total, n_changed = 10 ** 6, 0
    for s in SAMPLES:
        set_tables(pn, start)
        pn.train_edges(model, s, 1, total, K, 0.025, 0.0, SEED, mode)
        want = [padded(T, dim) for T in start]
        if model == "bpr":
            orc.train_bpr_f32(g, want[0], dim, 0.025, total, s, s + 1, SEED)
        else:
            orc.train_edge_f32(g, model, want[0], want[-1], dim, K, 0.025, 0.0, total, s, s + 1, SEED)
        n_changed += check(pn, dim, start, want, "%s sample %d" % (model, s))
    assert n_changed > 0   # the samples really updated rows


# ---------------------------------------------------------------- C++ and Go pair kernels
def _one_pair(V, i):
    rng = np.random.default_rng(1000 + i)
    v, c = rng.integers(0, V, 2)
    return np.array([v], np.int32), np.array([c if c != v else (c + 1) % V], np.int32)


@pytest.mark.parametrize("mi", range(len(MODES)), ids=MODE_IDS)
@pytest.mark.parametrize("dim", [8, 128])
@pytest.mark.parametrize("K", [5, 10])
@pytest.mark.parametrize("sem", ["cpp", "go"])
def test_pair_routing(smore, sem, K, dim, mi):
    mode, tau = MODES[mi]
    go = sem == "go"
    g, pn = oracle_graph("pl100w.txt", 1, go), pronet(smore, "pl100w.txt", 1, go)
    start = rand_tables(g.V, dim, dim + K)
    pn.alloc_tables(dim, 2)
    if tau is not None:
        pn.set_hot_threshold(tau)
    for i in range(len(SAMPLES)):
        v, c = _one_pair(g.V, i)
        unit = 77 + i
        set_tables(pn, start)
        pn.train_pairs(v, c, K, 0.025, SEED, unit, mode)
        want = [padded(T, dim) for T in start]
        orc.update_pairs_f32(g, want[0], want[1], dim, v, c, K, 0.025, SEED, unit, go=go)
        assert check(pn, dim, start, want, "%s pair %d" % (sem, i)) > 0


# ---------------------------------------------------------------- Go record kernel
@pytest.mark.parametrize("mi", range(len(MODES)), ids=MODE_IDS)
@pytest.mark.parametrize("model,K,dim", [("line2", 5, 8), ("line2", 10, 300), ("bpr", 1, 64)])
def test_go_record_routing(smore, model, K, dim, mi):
    mode, tau = MODES[mi]
    fname, und = ("bip.txt", 0) if model == "bpr" else ("pl100w.txt", 1)
    g, pn = oracle_graph(fname, und, True), pronet(smore, fname, und, True)
    start = rand_tables(g.V, dim, dim + K)
    pn.alloc_tables(dim, 2)
    if tau is not None:
        pn.set_hot_threshold(tau)
    lam = 0.01 if model == "bpr" else 0.0
    total, n_changed = 10 ** 6, 0
    for s in SAMPLES:
        set_tables(pn, start)
        pn.train_edges(model, s, 1, total, K, 0.025, lam, SEED, mode)
        want = [padded(T, dim) for T in start]
        orc.go_train_f32(g, model, want[0], want[1], dim, K, 0.025, lam, total, s, s + 1, SEED)
        n_changed += check(pn, dim, start, want, "go %s sample %d" % (model, s))
    assert n_changed > 0


# ---------------------------------------------------------------- WARP
@pytest.mark.parametrize("mode", ["atomic", "hogwild"])
@pytest.mark.parametrize("dim", [5, 128])
def test_warp_routing(smore, dim, mode):
    g = ws.graph("bip.txt")
    pn = pronet(smore, "bip.txt", 0, nm="no_degrees")
    start = [ws.lcg_table(g.V, dim).astype(np.float32)]
    pn.alloc_tables(dim, 1)
    n_changed = 0
    for s in SAMPLES:
        set_tables(pn, start)
        pn.train_warp(s, 1, 10 ** 6, 0.05, SEED, mode)
        want = [ws.padded(start[0], dim)]
        ws.run(g, want[0], 0.05, 10 ** 6, s, s + 1, SEED)
        n_changed += check(pn, dim, start, want, "warp sample %d" % s)
    assert n_changed > 0
