"""Exact update accounting of the lossless parallel scatter modes over MANY
samples: the atomic scatter, and the hybrid scatter with every row hot (with
and without LDS write-combining), must apply every sample's update exactly
once, whatever the interleaving.  Needs an MI355X.

Each case runs one multi-sample launch from fixed tables and compares the
result with the linearised fp64 reference L = T0 + sum_s D_s(T0)
(tests/linear_spec.py), which does not depend on the order of the samples.
With alpha0 = 2e-4 the launch differs from L by second-order terms and fp32
rounding only; a dropped, doubled or misrouted sample is first order.

  tol = 4 x gap,  gap = max |S - L| of the oracle's serial fp32 spec S over
                  two CPU orders (records in order, records reversed)

computed per case from the reference alone, never from the GPU's output.  The
preconditions that make `tol` discriminating (every sample moves a row by at
least 8 tol, ...) are asserted for every case of CASES on the CPU
(tests/test_linear_spec_cpu.py imports CASES and reference()).

What the launches exercise: the chunk hand-out and its tail (n is prime), the
two-sample pipeline, BPR's loop, the LDS write-combining with its drain
schedule and the end-of-kernel flush, the pair kernel's slices and W runs,
bucket launches of a block cell, and the double-buffered record chunks.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest

from oracle import oracle as orc
from tests import linear_spec as ls
from tests.block_spec import BlockSpec

pytestmark = pytest.mark.gpu

SEED = 20251015
ALPHA0 = 2e-4
TOTAL = 10 ** 12
BEGIN = 12345
V = 8192
N, N_WIDE = 4099, 1031      # primes: never a multiple of the groups per block
UNIT = 77                   # the pair calls' unit offset
CH_ROUNDS = 128             # train_kernels.h
# smore_set_write_combine takes any drain interval, but a row is combined only
# while (resident groups) x p(row) x interval <= SH_STALE_MAX = 65536
# (hot_maps.cpp): 4096 rounds keep the planted hubs (M p ~ 6) in the set and
# are far more than the ~8 rounds of a launch here, so the end-of-kernel flush
# carries every combined delta.
LONG_DRAIN = 4096


# ---------------------------------------------------------------- graphs
@functools.lru_cache(maxsize=None)
def edges(kind):
    """Directed edge slots (src, dst), unit weights.  "ring": undirected, a
    ring, ~3V random chords, 4096 edges from 16 planted hubs (each edge pushed
    both ways).  "bip": 4096 users -> 4096 items, 6 random items per user (no
    planted hubs: BPR's five rounds on a hub item make the second-order term
    of the ordering gap several times the rounding, at no gain in coverage --
    4099 samples over 4096 users and items already share rows)."""
    rng = np.random.default_rng(SEED)
    if kind == "ring":
        a = [np.arange(V), rng.integers(0, V, 3 * V), np.repeat(rng.choice(V, 16, replace=False), 256)]
        b = [(np.arange(V) + 1) % V, rng.integers(0, V, 3 * V), rng.integers(0, V, 4096)]
        a, b = np.concatenate(a), np.concatenate(b)
        keep = a != b
        a, b = a[keep], b[keep]
        src = np.stack([a, b], axis=1).ravel()
        dst = np.stack([b, a], axis=1).ravel()
    else:
        U = V // 2
        src = np.repeat(np.arange(U), 6)
        dst = U + rng.integers(0, U, 6 * U)
    return src.astype(np.int32), dst.astype(np.int32)


@functools.lru_cache(maxsize=None)
def oracle_graph(kind, go):
    src, dst = edges(kind)
    w = np.ones(len(src))
    if go:
        return orc.GoGraph(V, src, dst, w)
    return orc.Graph(V, src, dst, w, "out_degrees", "no_degrees" if kind == "bip" else "degrees")


# family -> (graph kind, Go semantics, tables, train_edges model, rule, rule kwargs, rate schedule)
FAMILIES = {
    "line2": ("ring", False, 2, "line2", "cpp", {}, "line"),
    "line1": ("ring", False, 1, "line1", "cpp", {"shared": True}, "line"),
    "mf": ("bip", False, 1, "mf", "cpp", {"shared": True, "mf": True, "reg": 0.01}, "mf"),
    "bpr": ("bip", False, 1, "bpr", "bpr", {}, "mf"),
    "go_line2": ("ring", True, 2, "line2", "go", {}, "go"),
    "go_bpr": ("bip", True, 2, "bpr", "gobpr", {"lam": 0.01}, "go"),
    "pairs_cpp": ("ring", False, 2, None, "cpp", {}, "fixed"),
    "pairs_go": ("ring", True, 2, None, "go", {}, "fixed"),
    "pairs_plain": ("ring", False, 2, None, "cpp", {}, "fixed"),
    "block": ("ring", False, 2, None, "cpp", {}, "line"),
}


# Where ls.preconditions() cannot hold as it stands, the weaker form that does
# and why (asserted on the CPU for the family's cases; `check` and tol = 4 gap
# are the same for every family).
PRECONDITIONS = {
    # No row is touched twice by construction, and K = 0 leaves one context id.
    "pairs_plain": dict(want_multi=False, want_repeat=False),
    # UpdateBPRPair: the fastSigmoid bucket flips of five rounds make gap ~ 4e-6
    # (LINE-2: 9e-7), so tol ~ 2e-5.  A sample still moves its positive item's
    # row by five rounds' worth, >= 2 tol -- lost or doubled it shows above tol
    # even on top of rounding as large as tol -- but not by 8 tol; a negative
    # item's row takes one step of g * w_u ~ 2.5e-5, about tol by the rule
    # itself, so only the touches of the user's and the positive's rows count.
    "bpr": dict(sample_factor=2.0, touch_cols=(0, 1)),
    # Go UpdateBPRPair: one sigma(neg - pos) gates the whole sample; with
    # neg - pos ~ N(0, 0.94^2) at d = 64 about 3-4 % of the samples have
    # sigma < 0.14 and move no row by 8 tol.  Such a sample lost is invisible
    # to any comparison of values; the launch errors looked for drop samples
    # whatever their gate, and k of them all gated has probability < 0.05^k.
    # One negative: a repeat needs j == i (pinned in serial mode, test_gpu_go.py).
    "go_bpr": dict(weak_samples=0.05, want_repeat=False),
}


def pair_ids(n, plain):
    """Caller pairs.  plain: v and c prefixes of two permutations (no row
    touched twice).  Else 5 single pairs, then runs of 8 pairs with one v over
    the first half, then single pairs; an eighth of the contexts are hub
    vertices, so that negatives repeat them.  The 5 leading pairs keep the runs off the
    multiples of 8, hence off the slice boundaries of CH_ROUNDS records."""
    rng = np.random.default_rng(SEED + 1)
    if plain:
        return rng.permutation(V)[:n].astype(np.int32), rng.permutation(V)[:n].astype(np.int32)
    v = rng.integers(0, V, n)
    runs = (n // 2) // 8
    v[5:5 + 8 * runs] = np.repeat(rng.integers(0, V, runs), 8)
    src, _ = edges("ring")
    hubs = np.argsort(-np.bincount(src, minlength=V), kind="stable")[:16]
    c = np.where(rng.random(n) < 0.125, hubs[rng.integers(0, 16, n)], rng.integers(0, V, n))
    return v.astype(np.int32), c.astype(np.int32)


def slice_len(dim, n, max_blocks=None):
    """Records per group slice of a train_pairs call of n pairs (train.cpp
    train_pairs_core / edge_grid; the device has more block slots than the
    V/16 concurrency cap allows here)."""
    gpb = 256 // orc.lane_width((dim + 3) // 4 * 4)
    grid = min(-(-(V // 16) // gpb), -(-n // gpb))
    if max_blocks:
        grid = min(grid, max_blocks)
    groups = grid * gpb
    return CH_ROUNDS if n >= groups * CH_ROUNDS else max(1, -(-n // groups))


Ref = namedtuple("Ref", "fam dim K n graph T0 records alphas rule kw lin gap tol touched skipped pairs neg_scale")


def tables(fam, dim, rows=V):
    rng = np.random.default_rng(SEED + dim)
    s = 0.5 * min(1.0, (64.0 / dim) ** 0.5)
    return [((rng.random((rows, dim)) - 0.5) * 2 * s).astype(np.float32) for _ in range(FAMILIES[fam][2])]


@functools.lru_cache(maxsize=None)
def block_spec(part):
    return BlockSpec(oracle_graph("ring", False), 2, part, 5)


@functools.lru_cache(maxsize=None)
def reference(fam, dim, K, n, extra=None):
    """Graph, records, L, gap and tol of one (family, dim, K, n): CPU only,
    shared by the modes and grid shapes."""
    kind, go, ntab, model, rule, kw, sched = FAMILIES[fam]
    kw = dict(kw)
    g = oracle_graph(kind, go)
    pairs, neg_scale, rows = None, 1.0, V
    if fam in ("line2", "line1", "mf"):
        rec = orc.sample_line(g, SEED, BEGIN, n, K)
    elif fam == "bpr":
        rec = orc.sample_bpr(g, SEED, BEGIN, n)
    elif fam in ("go_line2", "go_bpr"):
        rec = orc.go_sample(g, SEED, BEGIN, n, 1 if fam == "go_bpr" else K)
    elif fam == "block":
        spec = block_spec(extra[0])
        rec = spec.draw(extra[1], SEED, BEGIN, n, K)
        neg_scale = spec.neg_w[extra[1]]
        kw["neg_scale"] = neg_scale
        rows = V + spec.H
    else:
        pairs = pair_ids(n, fam == "pairs_plain")
        rec = ls.pair_records(g, pairs[0], pairs[1], K, SEED, UNIT)
    T0 = tables(fam, dim)
    if rows > V:      # the hub slots: rows V .. V + H of C start as the hub rows
        T0[1] = np.concatenate([T0[1], T0[1][block_spec(extra[0]).hubs]])
    alphas = ls.rates(sched, BEGIN, n, ALPHA0, TOTAL)
    lin = ls.linear(T0, rec, rule, alphas, **kw)

    # the serial fp32 spec in two orders
    def start():
        return [ls.padded(T) for T in T0]
    a, b = start(), start()
    if fam in ("line2", "line1", "mf", "block"):
        m = model or "line2"
        reg = kw.get("reg", 0.0)
        if fam == "block":
            orc.train_records_f32(m, a[0], a[-1], rec, K, ALPHA0, reg, TOTAL, BEGIN, neg_scale)
        else:
            orc.train_edge_f32(g, m, a[0], a[-1], dim, K, ALPHA0, reg, TOTAL, BEGIN, BEGIN + n, SEED)
        orc.train_records_f32(m, b[0], b[-1], rec[::-1], K, ALPHA0, reg, TOTAL, BEGIN, neg_scale)
    elif fam == "bpr":
        mid = BEGIN + n // 2
        orc.train_bpr_f32(g, a[0], dim, ALPHA0, TOTAL, BEGIN, BEGIN + n, SEED)
        orc.train_bpr_f32(g, b[0], dim, ALPHA0, TOTAL, mid, BEGIN + n, SEED)
        orc.train_bpr_f32(g, b[0], dim, ALPHA0, TOTAL, BEGIN, mid, SEED)
    elif fam in ("go_line2", "go_bpr"):
        mid, lam = BEGIN + n // 2, kw.get("lam", 0.0)
        orc.go_train_f32(g, model, a[0], a[1], dim, K, ALPHA0, lam, TOTAL, BEGIN, BEGIN + n, SEED)
        orc.go_train_f32(g, model, b[0], b[1], dim, K, ALPHA0, lam, TOTAL, mid, BEGIN + n, SEED)
        orc.go_train_f32(g, model, b[0], b[1], dim, K, ALPHA0, lam, TOTAL, BEGIN, mid, SEED)
    else:
        orc.update_pairs_f32(g, a[0], a[1], dim, pairs[0], pairs[1], K, ALPHA0, SEED, UNIT, go=go)
        if go:        # the oracle's Go fp32 rule takes no records: the numpy fp32 rule, reversed
            ls.rule_f32(b, rec[::-1], rule, alphas[::-1])
        else:         # records 0 .. n-1 of a run that starts at 0 all have the rate alpha0
            orc.train_records_f32("line2", b[0], b[1], rec[::-1], K, ALPHA0, 0.0, TOTAL, 0)
    gap = ls.gap(lin.L, [a, b])
    return Ref(fam, dim, K, n, g, T0, rec, alphas, rule, kw, lin, gap, 4 * gap, lin.touched(),
               int((~ls.live(rec)).sum()), pairs, neg_scale), (a, b)


# ---------------------------------------------------------------- the case table
# mode: (scatter mode, hot threshold, write-combine (rows, drain interval) or None)
ATOMIC = ("atomic", None, None)
COMBINE = ("hybrid", 0.0, (128, 0))
MODES = {"atomic": ATOMIC, "hybrid-wc": COMBINE, "hybrid-wc-drain1": ("hybrid", 0.0, (128, 1)),
         "hybrid-wc-flush": ("hybrid", 0.0, (128, LONG_DRAIN)), "hybrid-nowc": ("hybrid", 0.0, (0, 0)),
         "hogwild": ("hogwild", None, None), "hybrid-cold": ("hybrid", 1e30, None)}
Case = namedtuple("Case", "fam dim K n mode env extra")


def _cases():
    out = []

    def add(fam, dim, K, modes, n=N, env=(), extra=None):
        out.extend(Case(fam, dim, K, n, m, tuple(env), extra) for m in modes)
    both = ("atomic", "hybrid-wc")
    add("line2", 64, 5, ("atomic", "hybrid-wc", "hybrid-wc-drain1", "hybrid-wc-flush", "hybrid-nowc"))
    add("line2", 64, 5, both, env=[("SMORE_MAX_BLOCKS", "3")])
    add("line2", 64, 5, both, env=[("SMORE_DRAW_CHUNK", "1024")])
    for dim, K, n in ((8, 17, N), (20, 3, N), (128, 9, N), (300, 9, N_WIDE)):
        add("line2", dim, K, both, n=n)
    add("line1", 64, 5, both)
    add("mf", 12, 5, ("atomic",))
    for dim in (64, 128):
        add("bpr", dim, 5, ("atomic",))
        add("bpr", dim, 5, ("hybrid-nowc",), env=[("SMORE_BPR_SCATTER", "tagged")])
        add("bpr", dim, 5, ("hybrid-wc",), env=[("SMORE_BPR_SCATTER", "tagged"), ("SMORE_BPR_COMBINE", "1")])
    add("go_line2", 64, 5, both)
    add("go_bpr", 64, 1, both)
    for fam in ("pairs_cpp", "pairs_go"):
        for dim, K in ((64, 5), (128, 10)):
            add(fam, dim, K, both)
            add(fam, dim, K, both, env=[("SMORE_MAX_BLOCKS", "1")])
    add("pairs_plain", 64, 0, ("hogwild", "hybrid-cold"))
    for block in (0, 3):
        add("block", 32, 5, ("atomic", "hybrid-wc"), extra=(0, block))
    return out


CASES = _cases()


def case_id(c):
    return "-".join([c.fam, "d%d" % c.dim, "K%d" % c.K, c.mode] + ["%s=%s" % (k.replace("SMORE_", ""), v) for k, v in c.env]
                    + (["block%d" % c.extra[1]] if c.extra else []))


def ref_key(c):
    return (c.fam, c.dim, c.K, c.n, c.extra)


# ---------------------------------------------------------------- the GPU side
@pytest.fixture(scope="module")
def smore():
    import smore_amd
    return smore_amd


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_conservation(smore, monkeypatch, case):
    ref, _ = reference(*ref_key(case))
    env = dict(case.env)
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    try:
        got, L, T0, touched = _launch(smore, case, ref, env)
    except smore._lib.SmoreError as e:
        # a failed launch may have faulted the GPU: nothing more runs on it in this session
        pytest.exit("%s: %s" % (case_id(case), e), returncode=3)
    print("CONSERVATION %s gap %.3g tol %.3g residual %.3g = %.2f gap" % (
        case_id(case), ref.gap, ref.tol, ls.residual(got, L), ls.residual(got, L) / ref.gap))
    ls.check(got, T0, L, ref.tol, touched)


def _launch(smore, case, ref, env):
    """The case's launch from ref.T0; returns the tables read back and the
    reference (L, T0, touched rows) in their layout."""
    kind, go, ntab, model, _, kw, _ = FAMILIES[case.fam]
    mode, tau, wc = MODES[case.mode]
    src, dst = edges(kind)
    pn = smore.ProNet(0)
    pn.SetNegativeMethod("no_degrees" if kind == "bip" else "degrees")
    pn.set_graph_edges(V, src, dst, None)
    if go:
        pn.set_semantics("go")
    pn.alloc_tables(case.dim, ntab)
    for t in range(ntab):
        pn.set_table(t, ref.T0[t][:V])
    if tau is not None:
        pn.set_hot_threshold(tau)
    if wc is not None:
        pn.set_write_combine(*wc)
    skipped0 = pn.skipped()
    if case.fam == "block":
        part, block = case.extra
        pn.block_setup("line2", 2, part, case.K, mode)
        H, first, hub_rows, _ = pn.block_hubs()
        assert H == ref.T0[1].shape[0] - V and first == V and list(hub_rows) == list(block_spec(part).hubs)
        np.testing.assert_array_equal(pn.block_sample_edges(block, SEED, BEGIN, case.n, case.K), ref.records)
        np.testing.assert_allclose(pn.block_neg_scale(block), ref.neg_scale, rtol=1e-6)
        pn.block_hubs_load()
        pn.block_train_edges(block, BEGIN, case.n, TOTAL, case.K, ALPHA0, SEED, mode)
        pn.block_hubs_store()
    elif ref.pairs is not None:
        if case.fam != "pairs_plain":
            # some run of 8 equal v lies across a slice boundary
            sl = slice_len(case.dim, case.n, int(env["SMORE_MAX_BLOCKS"]) if "SMORE_MAX_BLOCKS" in env else None)
            if "SMORE_MAX_BLOCKS" in env:
                assert sl == CH_ROUNDS
            v, runs = ref.pairs[0], (case.n // 2) // 8
            cut = np.arange(sl, case.n, sl)
            cut = cut[(cut > 5) & (cut < 5 + 8 * runs) & ((cut - 5) % 8 != 0)]     # inside a run of pair_ids()
            assert cut.size and (v[cut] == v[cut - 1]).all(), "no run straddles a slice boundary (slice %d)" % sl
        pn.train_pairs(ref.pairs[0], ref.pairs[1], case.K, ALPHA0, SEED, UNIT, mode)
    else:
        pn.train_edges(model, BEGIN, case.n, TOTAL, case.K, ALPHA0, kw.get("reg", kw.get("lam", 0.0)), SEED, mode)
    got = [pn.get_table(t) for t in range(ntab)]
    assert pn.last_mode() == mode
    assert pn.skipped() - skipped0 == ref.skipped
    if mode == "hybrid" and tau == 0.0 and case.fam != "block":   # a cell's tags are per block, not counted here
        assert sum(pn.hot_rows()) > 0
    if wc is not None and wc[0] > 0 and case.fam != "block":
        rows, drain = pn.write_combine_info()
        assert rows > 0
        if wc[1] > 0:
            assert drain == wc[1]
    pn.close()

    L, T0, touched = ref.lin.L, ref.T0, ref.touched
    if case.fam == "block" and L[1].shape[0] > V:
        # the slots were stored back into the hub rows (no record names a hub row itself)
        hubs = np.asarray(block_spec(case.extra[0]).hubs)
        Lc, Tc = L[1][:V].copy(), T0[1][:V]
        Lc[hubs] = L[1][V:]
        slots = touched[1][touched[1] >= V] - V
        L, T0 = [L[0], Lc], [T0[0], Tc]
        touched = [touched[0], np.union1d(touched[1][touched[1] < V], hubs[slots])]
    return got, L, T0, touched
