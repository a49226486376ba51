"""tests/linear_spec.py proven on the CPU: its rules are the oracle's fp64
rules, the linearised reference is order independent, the restated pair
negatives are the oracle's, the preconditions of `check` hold for every case
of tests/test_gpu_conservation.py (its case table is imported, not copied),
`check` rejects the mutants a lossy kernel would produce and accepts both
CPU fp32 orders."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import linear_spec as ls
from tests import test_gpu_conservation as gc
from tests.test_gpu_conservation import ALPHA0, BEGIN, SEED, TOTAL, UNIT, V

REF_KEYS = sorted({gc.ref_key(c) for c in gc.CASES}, key=repr)
EPS = 1e-12


def f64(tabs):
    return [np.array(T, np.float64) for T in tabs]


def one_sample_L(T0, rec, alpha, rule, kw):
    L = f64(T0)
    for (t, r), d in ls.sample_delta(T0, rec, alpha, rule, **kw).items():
        L[t][r] += d
    return L


def pick(rec, mask, plain=2, special=3):
    """A few plain sample indices and the first `special` under `mask`."""
    idx = list(np.flatnonzero(ls.live(rec) & ~mask)[:plain]) + list(np.flatnonzero(ls.live(rec) & mask)[:special])
    return idx, int(mask.sum())


def repeats(rec, shared):
    """Samples with a repeated context id (or, shared table, the source among them)."""
    s = np.sort(rec[:, 1:], axis=1)
    m = (s[:, 1:] == s[:, :-1]).any(axis=1)
    if shared:
        m |= (rec[:, :1] == rec[:, 1:]).any(axis=1)
    return m


# ---------------------------------------------------------------- the rules are the oracle's
@pytest.mark.parametrize("fam,dim,K", [("line2", 64, 5), ("line2", 20, 17), ("line1", 64, 5), ("mf", 12, 5)])
def test_rule_cpp_equals_oracle_f64(fam, dim, K):
    kind, _, ntab, model, rule, kw, sched = gc.FAMILIES[fam]
    g = gc.oracle_graph(kind, False)
    count = 60000
    rec = orc.sample_line(g, SEED, BEGIN, count, K)
    idx, nspecial = pick(rec, repeats(rec, ntab == 1))
    assert nspecial > 0
    T0 = gc.tables(fam, dim)
    for i in idx:
        s = BEGIN + int(i)
        want = f64(T0)
        orc.train_edge_f64(g, model, want[0], want[-1], K, ALPHA0, kw.get("reg", 0.0), TOTAL, s, s + 1, SEED)
        alpha = ls.rates(sched, s, 1, ALPHA0, TOTAL)[0]
        for Lt, Wt, Tt in zip(one_sample_L(T0, rec[i], alpha, rule, kw), want, T0):
            assert np.abs(Lt - Wt).max() <= EPS and (Wt != Tt).any()


def test_rule_bpr_equals_oracle_f64():
    g = gc.oracle_graph("bip", False)
    rec = orc.sample_bpr(g, SEED, BEGIN, 60000)
    idx, nspecial = pick(rec, repeats(rec, True))
    assert nspecial > 0
    T0 = gc.tables("bpr", 64)
    for i in idx:
        s = BEGIN + int(i)
        want = f64(T0)
        orc.train_bpr_f64(g, want[0], ALPHA0, TOTAL, s, s + 1, SEED)
        L = one_sample_L(T0, rec[i], ls.rates("mf", s, 1, ALPHA0, TOTAL)[0], "bpr", {})
        assert np.abs(L[0] - want[0]).max() <= EPS and (want[0] != T0[0]).any()


@pytest.mark.parametrize("fam,K", [("go_line2", 5), ("go_bpr", 1)])
def test_rule_go_equals_oracle_f64(fam, K):
    kind, _, _, model, rule, kw, sched = gc.FAMILIES[fam]
    g = gc.oracle_graph(kind, True)
    rec = orc.go_sample(g, SEED, BEGIN, 200000, K)
    # Go UpdatePair: a negative equal to the context; Go BPR: j == i
    idx, nspecial = pick(rec, (rec[:, 2:] == rec[:, 1:2]).any(axis=1))
    assert nspecial > 0
    T0 = gc.tables(fam, 64)
    for i in idx:
        s = BEGIN + int(i)
        want = f64(T0)
        orc.go_train_f64(g, model, want[0], want[1], K, ALPHA0, kw.get("lam", 0.0), TOTAL, s, s + 1, SEED)
        L = one_sample_L(T0, rec[i], ls.rates(sched, s, 1, ALPHA0, TOTAL)[0], rule, kw)
        for Lt, Wt, Tt in zip(L, want, T0):
            assert np.abs(Lt - Wt).max() <= EPS and (Wt != Tt).any()


# ---------------------------------------------------------------- pair negatives
@pytest.mark.parametrize("go", [False, True], ids=["cpp", "go"])
@pytest.mark.parametrize("K", [5, 10])
def test_pair_negatives_reproduce_oracle(go, K):
    """The restated negatives, run serially through the fp64 rule, are
    orc_update_pairs_f64 over 3000 pairs (and so is each rule on pairs)."""
    g = gc.oracle_graph("ring", go)
    n, dim = 3000, 16
    v, c = gc.pair_ids(n, False)          # runs of equal v, hub contexts (negatives repeat them)
    T0 = gc.tables("pairs_cpp", dim)
    want = f64(T0)
    orc.update_pairs_f64(g, want[0], want[1], v, c, K, 0.025, SEED, UNIT, go=go)
    rec = ls.pair_records(g, v, c, K, SEED, UNIT)
    got = ls.serial_f64(f64(T0), rec, "go" if go else "cpp", np.full(n, 0.025))
    for a, b in zip(got, want):
        assert np.abs(a - b).max() <= EPS
    # one pair: the linearised delta is the oracle's update
    one = f64(T0)
    orc.update_pairs_f64(g, one[0], one[1], v[:1], c[:1], K, 0.025, SEED, UNIT, go=go)
    for a, b in zip(one_sample_L(T0, rec[0], 0.025, "go" if go else "cpp", {}), one):
        assert np.abs(a - b).max() <= EPS


def test_pair_negatives_cross_the_unit_block():
    """Pair i of a later 2^20-block draws from unit + i // 2^20 (checked on the ids only)."""
    g = gc.oracle_graph("ring", False)
    K, n = 5, orc.PAIR_BLOCK + 3
    negs = ls.pair_negatives(g, n, K, SEED, UNIT)
    np.testing.assert_array_equal(negs[orc.PAIR_BLOCK:], ls.pair_negatives(g, 3, K, SEED, UNIT + 1))
    np.testing.assert_array_equal(negs[:3], ls.pair_negatives(g, 3, K, SEED, UNIT))


# ---------------------------------------------------------------- order independence
def test_linear_is_serial_without_conflicts():
    ref, _ = gc.reference("pairs_plain", 64, 0, gc.N, None)
    assert all(len(np.unique(ref.pairs[t])) == gc.N for t in range(2))
    got = ls.serial_f64(f64(ref.T0), ref.records, ref.rule, ref.alphas)
    for a, b in zip(got, ref.lin.L):
        assert np.abs(a - b).max() <= EPS
    # LINE-2 records that share no row, in both orders
    ref, _ = gc.reference("line2", 64, 5, gc.N, None)
    seen, keep = [set(), set()], []
    for i, r in enumerate(ref.records):
        ids = [{int(r[0])}, {int(x) for x in r[1:]}]
        if r[1] >= 0 and len(ids[1]) == len(r) - 1 and not (ids[0] & seen[0]) and not (ids[1] & seen[1]):
            keep.append(i)
            seen[0] |= ids[0]
            seen[1] |= ids[1]
    assert len(keep) > 300
    rec, al = ref.records[keep], ref.alphas[keep]
    L = ls.linear(ref.T0, rec, "cpp", al).L
    for order in (slice(None), slice(None, None, -1)):
        got = ls.serial_f64(f64(ref.T0), rec[order], "cpp", al[order])
        for a, b in zip(got, L):
            assert np.abs(a - b).max() <= EPS


# ---------------------------------------------------------------- preconditions and both fp32 orders
@pytest.mark.parametrize("key", REF_KEYS, ids=lambda k: "-".join(str(x) for x in k if x is not None))
def test_preconditions_and_cpu_orders(key):
    ref, runs = gc.reference(*key)
    assert ref.gap > 0 and ref.tol == 4 * ref.gap
    ls.preconditions(ref.lin, ref.records, ref.tol, shared=len(ref.T0) == 1, **gc.PRECONDITIONS.get(ref.fam, {}))
    dim = ref.dim
    for S in runs:        # `check` accepts the legitimate fp32 results
        ls.check([T[:, :dim] for T in S], ref.T0, ref.lin.L, ref.tol, ref.touched)
    assert ref.skipped == int((ref.records[:, 1] < 0).sum())


# ---------------------------------------------------------------- the check can fail
def _mutated(ref, S, changes):
    """The fp32 result S plus `changes` = [(sign, {(table, row): delta})]."""
    out = [np.array(T[:, :ref.dim], np.float64) for T in S]
    for sign, delta in changes:
        for (t, r), d in delta.items():
            out[t][r] += sign * d
    return [T.astype(np.float32) for T in out]


def _rejected(ref, got):
    with pytest.raises(AssertionError):
        ls.check(got, ref.T0, ref.lin.L, ref.tol, ref.touched)


def test_check_rejects_mutants():
    ref, (S, _) = gc.reference("line2", 64, 5, gc.N, None)
    ls.check([T[:, :ref.dim] for T in S], ref.T0, ref.lin.L, ref.tol, ref.touched)

    def delta(s):
        return ls.sample_delta(ref.T0, ref.records[s], ref.alphas[s], ref.rule, **ref.kw)
    lv = np.flatnonzero(ls.live(ref.records))
    weakest = int(lv[np.argmin(ref.lin.sample_max[lv])])       # the sample that moves its rows least
    _rejected(ref, _mutated(ref, S, [(-1, delta(weakest))]))   # left out
    _rejected(ref, _mutated(ref, S, [(+1, delta(weakest))]))   # applied twice
    tail = [s for s in range(gc.N - gc.N % 16, gc.N) if ref.records[s, 1] >= 0]
    assert 0 < len(tail) < 16
    _rejected(ref, _mutated(ref, S, [(-1, delta(s)) for s in tail]))     # the last n mod 16 samples
    # one row touch left out: the smallest one the preconditions call visible
    lin = ref.lin
    ok = np.flatnonzero(lin.touch_max >= 2 * ref.tol)
    j = int(ok[np.argmin(lin.touch_max[ok])])
    key = (int(lin.touch_table[j]), int(lin.touch_row[j]))
    _rejected(ref, _mutated(ref, S, [(-1, {key: delta(int(lin.touch_sample[j]))[key]})]))
    # an untouched row that changed by one ulp
    got = [T[:, :ref.dim].copy() for T in S]
    free = np.setdiff1d(np.arange(V), ref.touched[0])[0]
    got[0][free, 0] = np.nextafter(got[0][free, 0], np.float32(1))
    _rejected(ref, got)


def test_check_rejects_a_doubled_run():
    """All W updates of one run of pairs applied twice (a run's W delta
    flushed twice at a slice boundary)."""
    ref, (S, _) = gc.reference("pairs_cpp", 64, 5, gc.N, None)
    v = ref.pairs[0]
    assert (v[5:13] == v[5]).all() and v[13] != v[5]
    w = np.zeros(ref.dim)
    for s in range(5, 13):
        w += ls.sample_delta(ref.T0, ref.records[s], ref.alphas[s], ref.rule, **ref.kw)[(0, int(v[5]))]
    _rejected(ref, _mutated(ref, S, [(+1, {(0, int(v[5])): w})]))
