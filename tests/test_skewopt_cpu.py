"""Skew-OPT on the CPU: the rule's spec (tests/c/skewopt_spec.c) against the
reference's own runs (tests/golden/updates_skewopt.npz, e2e_skewopt_bip.npz;
how they were made: DESIGN.md 6 item 8 and 12c), the conditions the committed
trials must meet, the g == 0 definition of the fp32 rule, and where the fp32
and the fp64 instance of the rule part ways."""
import numpy as np
import pytest

from tests import skewopt_spec as ss

Z = ss.gold("updates_skewopt")


def test_lib_binding_declares_skewopt():
    from smore_amd import _lib
    sig = _lib.lib._signatures
    assert sig["smore_train_skewopt"] == sig["smore_train_skewopt_async"]
    assert len(sig["smore_train_skewopt"][1]) == 10 and len(sig["smore_skewopt_stats"][1]) == 3
    assert len(sig["smore_init_table_glibc_offset"][1]) == 4
    import smore_amd
    assert "SPR" in smore_amd.__all__ and hasattr(smore_amd.ProNet, "train_skewopt")
    assert hasattr(smore_amd.ProNet, "skewopt_stats") and hasattr(smore_amd.ProNet, "init_table_glibc_offset")


@pytest.mark.parametrize("tag", ss.tags(Z))
def test_fp64_spec_reproduces_single_updates_bit_exact(tag):
    tr = ss.Trials(Z, tag)
    assert int(Z[tag + "_others_unchanged"][0]) == 1
    for t in range(tr.n):
        s, gated, up, ids, passed, T0, want = tr.trial(t)
        T = T0.copy()
        r = tr.run(T, s)
        assert r.skipped == 0 and np.array_equal(r.rec[0], ids), (tag, t)
        assert np.array_equal(r.trace[0] >= 0, passed.astype(bool)), (tag, t)
        assert r.passed == up == int(passed.sum()) and r.updated == (up > 0)
        # `want` is T0 with the 18 rows the reference left: every other row is unchanged
        assert np.array_equal(T, want), (tag, t)


def test_fp64_spec_reproduces_end_to_end_bit_exact():
    z = ss.gold("e2e_skewopt_bip")
    dim, st, eta, seed = (int(x) for x in z["meta"])
    alpha, xi, omega = (float(x) for x in z["meta_f"])
    g = ss.graph("bip.txt")
    assert np.array_equal(z["W0"].astype(np.float32), ss.glibc_table(g.V, dim))
    T = z["W0"].copy()
    ss.run(g, T, alpha, xi, omega, eta, st * 10 ** 6, 0, st * 10 ** 6, seed)
    assert np.array_equal(T, z["W"])


def test_committed_trials_meet_their_conditions():
    total = mixed = interior = eiv = eji = ejv = ejj = all_gated = 0
    for tr, t in ss.all_trials():
        s, gated, up, ids, passed, T0, _want = tr.trial(t)
        T = T0.copy()
        r = tr.run(T, s)
        assert r.gmin > 0.0, (tr.tag, t)            # no trial has g == 0
        total += 1
        mixed += 0 < int(passed.sum()) < 16
        interior += bool((r.kind[0] == 2).any())
        v, i, js = int(ids[0]), int(ids[1]), [int(x) for x in ids[2:]]
        eiv += i == v
        eji += i in js
        ejv += v in js
        ejj += len(set(js)) < 16
        if gated:
            assert up == 0 and r.passed == 0 and r.updated == 0 and np.array_equal(T, T0)
            assert tr.dim * tr.c * tr.c > tr.xi + 2 * tr.omega
            assert v not in js and i not in js
            all_gated += 1
    assert mixed >= 0.1 * total and interior >= 0.1 * total, (mixed, interior, total)
    assert eiv >= 1 and eji >= 1 and ejv >= 1 and ejj >= 1, (eiv, eji, ejv, ejj)
    assert all_gated >= 3
    etas = {ss.Trials(Z, tag).eta for tag in ss.tags(Z)}
    assert etas == {1, 2, 3}
    assert any(ss.Trials(Z, tag).xi == 10.0 and ss.Trials(Z, tag).omega == 3.0 for tag in ss.tags(Z))


def test_decision_agreement_and_fp32_single_updates_within_1e5():
    """A trial whose fp32 decision trace (gate, clamp, sigmoid bucket per
    negative) differs from the fp64 one is left out, at most 5 % of them; every
    other trial's fp32 table is within 1e-5 absolute of the reference's."""
    out = ss.left_out()
    total = 0
    for tr, t in ss.all_trials():
        total += 1
        if (tr.tag, t) in out:
            continue
        s, _g, _up, _ids, _p, T0, want = tr.trial(t)
        T32 = ss.padded(T0.astype(np.float32), tr.dim)
        tr.run(T32, s)
        np.testing.assert_allclose(T32[:, :tr.dim], want, atol=1e-5, rtol=0, err_msg="%s trial %d" % (tr.tag, t))
        assert not T32[:, tr.dim:].any()
    print("left out", sorted(out), "of", total)
    assert len(out) <= 0.05 * total, (sorted(out), total)


def test_g_zero_is_the_limit_in_fp32():
    """f == xi exactly at every negative: the reference divides 0 by 0; the fp32
    rule takes chain as its limit.  The rate is 2^-20, so that the decays
    (factor 1 - 2^-20 * 0.01) round to nothing on the rows' 1 and 0.75 and row i
    keeps f == xi through all sixteen negatives.  eta >= 2: chain 0, gg 0, only
    the decays move the rows -- by hand, the table is unchanged, with 16 gates
    passed.  eta 1: chain 1, the first negative moves row i by
    ce = sig(0) / omega * alpha * T[v] and its own row by -ce."""
    g, dim, s, ids, xi, omega, alpha, seed = ss.gzero_case()
    v, i, j0 = int(ids[0]), int(ids[1]), int(ids[2])
    T0 = ss.gzero_table(g.V, dim, v, i, xi).astype(np.float32)
    for eta in (2, 3, 5):
        T = T0.copy()
        r = ss.run(g, T, alpha, xi, omega, eta, ss.TOTAL, s, s + 1, seed)
        assert r.gmin == 0.0 and r.passed == 16 and r.updated == 1 and (r.kind == 2).all()
        assert np.isfinite(T).all() and T.tobytes() == T0.tobytes()
    T = T0.copy()
    r = ss.run(g, T, alpha, xi, omega, 1, ss.TOTAL, s, s + 1, seed)
    assert r.gmin == 0.0 and r.passed == 16 and np.isfinite(T).all()
    ce = np.float32(np.float32(0.5) / np.float32(omega)) * np.float32(alpha)   # 0.5 / 0.5 * 2^-20: exact
    assert T[i, 0] > T0[i, 0] and (list(ids[2:]).count(j0) > 1 or T[j0, 0] == -ce)


def test_branch_divergence_of_fp32_and_fp64_is_a_margin_decision():
    """Where the fp32 and fp64 instances part ways on the 10^6-sample run -- a
    gate or a clamp decided differently (a different sigmoid bucket alone is no
    branch) -- the split is a rounding decision: up to that negative the runs took
    the same branches, and there the fp64 g is within the bound on |g32 - g64|
    that the tables' difference at that negative allows of the threshold (2 or
    -2) that the two decisions straddle.  Full agreement returns early."""
    z = ss.gold("e2e_skewopt_bip")
    dim, st, eta, seed = (int(x) for x in z["meta"])
    alpha, xi, omega = (float(x) for x in z["meta_f"])
    total = st * 10 ** 6
    g = ss.graph("bip.txt")
    A, B = z["W0"].copy(), ss.padded(z["W0"].astype(np.float32), dim)
    k64 = ss.run(g, A, alpha, xi, omega, eta, total, 0, total, seed).kind
    k32 = ss.run(g, B, alpha, xi, omega, eta, total, 0, total, seed).kind
    diff = np.nonzero((k64 != k32).any(1))[0]
    if len(diff) == 0:
        return   # full agreement: nothing to bound
    s = int(diff[0])
    n = int(np.nonzero(k64[s] != k32[s])[0][0])
    A, B = z["W0"].copy(), ss.padded(z["W0"].astype(np.float32), dim)
    ss.run(g, A, alpha, xi, omega, eta, total, 0, s, seed)
    ss.run(g, B, alpha, xi, omega, eta, total, 0, s, seed)
    # the tables as negative n of sample s finds them, and its g in both instances
    g64 = ss.run(g, A, alpha, xi, omega, eta, total, s, s + 1, seed, stop=n)
    g32 = ss.run(g, B, alpha, xi, omega, eta, total, s, s + 1, seed, stop=n)
    delta = np.abs(A - B[:, :dim]).max()
    big = max(np.abs(A).max(), np.abs(B).max())
    # f = sum_k wv_k (wi_k - wj_k): |df| <= d (delta * 2 big + big * 2 delta), plus the fp32
    # evaluation's own rounding, d + 2 operations of relative 2^-24 on terms <= 2 big^2;
    # g = (f - xi) / omega: two more roundings of relative 2^-24 on |f - xi| <= 2 d big^2 + xi
    df = dim * 4 * delta * big + (dim + 2) * 2.0 ** -24 * dim * 2 * big * big
    bound = (df + 2 * 2.0 ** -24 * (dim * 2 * big * big + xi)) / omega
    thr = min((2.0, -2.0), key=lambda t: abs(g64 - t))
    print("first split: sample %d negative %d g64 %.9g g32 %.9g delta %.3g bound %.3g" % (s, n, g64, g32, delta, bound))
    assert abs(g64 - thr) <= bound, (s, n, g64, g32, bound, delta)
