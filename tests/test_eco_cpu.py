"""The sampled-softmax choice (ECO) rule on the CPU: the spec (tests/c/eco_spec.c) against the
reference's own runs (tests/golden/updates_eco.npz, e2e_eco_bip.npz), the shared exponential
(smore_amd/csrc/exp32.h) and the interface's names.

  * exp32                                     : 2^-21 relative over [-20, 20]; +inf, 0 and NaN outside
  * fp64 spec vs every single-sample trial    : bit for bit (record, slots, rows)
  * fp64 spec vs the 10^6-sample run          : bit for bit, and the saved bytes
  * fp32 spec vs the trials                   : 1e-5 on every trial, none left out
"""
import math

import numpy as np
import pytest

from tests import eco_spec as es


def test_interface_names():
    import smore_amd
    from smore_amd import _lib
    sig = _lib.lib._signatures
    assert sig["smore_train_eco"] == sig["smore_train_eco_async"]
    assert len(sig["smore_train_eco"][1]) == 9 and len(sig["smore_eco_stats"][1]) == 3
    assert len(sig["smore_eco_records"][1]) == 7 and len(sig["smore_init_table_glibc_unscaled"][1]) == 4
    for m in ("train_eco", "eco_stats", "eco_records", "init_table_glibc_unscaled"):
        assert callable(getattr(smore_amd.ProNet, m))
    assert "ECO" in smore_amd.__all__
    for m in ("LoadEdgeList", "LoadFieldMeta", "Init", "Train", "SaveWeights"):
        assert callable(getattr(smore_amd.ECO, m))


def test_exp32_accuracy():
    """10^6 evenly spaced arguments of [-20, 20] against glibc's double exp: below 2^-21."""
    worst, at = es.exp32_worst(-20.0, 20.0, 10 ** 6)
    print("exp32: worst relative error %.4g = 2^%.2f at x = %.6f" % (worst, math.log2(worst), at))
    assert worst < 2.0 ** -21


def test_exp32_outside_the_range():
    """The header's statement: +inf above 88, +0 below -86, a NaN as it is, nothing subnormal."""
    tiny = float(np.finfo(np.float32).tiny)
    assert es.exp32(88.0) == pytest.approx(math.exp(88.0), rel=2.0 ** -21) and math.isfinite(es.exp32(88.0))
    for x in (np.nextafter(np.float32(88.0), np.float32(89.0)), 88.7, 89.0, 1e4, 3e38, float("inf")):
        assert es.exp32(x) == float("inf")
    assert es.exp32(-86.0) == pytest.approx(math.exp(-86.0), rel=2.0 ** -21) and es.exp32(-86.0) >= tiny
    for x in (np.nextafter(np.float32(-86.0), np.float32(-87.0)), -87.4, -104.0, -1e4, -3e38, float("-inf")):
        assert es.exp32(x) == 0.0 and math.copysign(1.0, es.exp32(x)) == 1.0
    assert math.isnan(es.exp32(float("nan")))
    assert es.exp32(0.0) == 1.0 and es.exp32(-0.0) == 1.0


@pytest.fixture(scope="module")
def fixtures():
    return es.all_trials()


def test_fp64_spec_reproduces_every_trial_bit_for_bit(fixtures):
    n = skipped = 0
    for F in fixtures.values():
        for t in range(F.n):
            s, slots, rec, T0, want = F.trial(t)
            W = T0.copy()
            r = F.run(W, s)
            np.testing.assert_array_equal(r.rec[0], rec, err_msg="%s %d" % (F.key, t))
            assert r.slots[0] == slots and r.skipped == (rec[0] < 0)
            assert W.tobytes() == want.tobytes(), (F.key, t)   # the named rows, every other row unchanged
            assert r.clean[0] == (-1 if rec[0] < 0 else es.is_clean(rec, F.K))
            n += 1
            skipped += int(rec[0] < 0)
    assert n == 82 and skipped == 6   # the directed toy load: an item has no out-edge


def test_committed_trials_cover_the_cases(fixtures):
    seen, n = {}, 0
    for F in fixtures.values():
        for t in range(F.n):
            n += 1
            for c in es.special_cases(F.trial(t)[2], F.K):
                seen[c] = seen.get(c, 0) + 1
    print("trials %d: %s" % (n, seen))
    for c in ("clean", "neg=v", "c2=v", "c1=c2", "dup-neg", "shared", "skip"):
        assert seen.get(c, 0) >= 1, c


def test_fp32_spec_within_1e5_of_the_reference_on_every_trial(fixtures):
    n, worst = 0, 0.0
    for F in fixtures.values():
        for t in range(F.n):
            s, _slots, _rec, T0, want = F.trial(t)
            n += 1
            W = es.padded(T0.astype(np.float32), F.dim)
            F.run(W, s)
            assert (W[:, F.dim:] == 0).all()
            worst = max(worst, float(np.abs(W[:, :F.dim] - want).max()))
            np.testing.assert_allclose(W[:, :F.dim], want, atol=1e-5, rtol=0, err_msg="%s %d" % (F.key, t))
    print("worst |fp32 spec - reference| over %d trials: %.3g" % (n, worst))
    assert n == 82


@pytest.fixture(scope="module")
def whole_run():
    name, gf, ff = es.E2E
    z = es.gold(name)
    g = es.graph(gf)
    field, _n = es.load_fields(g, ff)
    dim, st, K, seed = (int(x) for x in z["meta"])
    alpha, reg = (float(x) for x in z["meta_f"])
    W = z["W0"].copy()
    r = es.run(g, field, W, K, alpha, reg, st * 10 ** 6, 0, st * 10 ** 6, seed)
    W32 = es.padded(z["W0"].astype(np.float32), dim)
    es.run(g, field, W32, K, alpha, reg, st * 10 ** 6, 0, st * 10 ** 6, seed)
    return z, g, field, W, W32[:, :dim], r


def test_fp64_spec_reproduces_the_whole_run(whole_run):
    z, g, field, W, W32, r = whole_run
    np.testing.assert_array_equal(field, z["field"])
    assert r.skipped == 0
    assert W.tobytes() == z["W"].tobytes()
    gap = float(np.abs(W32 - z["W"]).max())
    print("max |spec32 - reference| = %.3g (max |reference| %.3g), clean samples %d of 10^6"
          % (gap, np.abs(z["W"]).max(), int((r.clean == 1).sum())))
    # at most 1e-4: the class and the CLI are held to the reference itself (test_gpu_eco.py)
    assert np.isfinite(W32).all() and gap <= es.E2E_GAP_BOUND


def test_glibc_stride_2_tables_are_the_reference_init(whole_run):
    z, g = whole_run[0], whole_run[1]
    W0, I0 = es.glibc_tables(g.V, z["W0"].shape[1])
    assert W0.tobytes() == z["W0"].tobytes() and I0.tobytes() == z["I0"].tobytes()
    assert np.abs(W0).max() > 0.49   # not divided by dim


def test_spec_writer_reproduces_the_saved_file(whole_run):
    z, g = whole_run[0], whole_run[1]
    text = es.save_lines(g, z["W"])
    assert text == z["saved"].tobytes()
    assert int(text.split()[0]) == g.V == len(text.decode().splitlines()) - 1


def test_recorded_spec_objective_is_what_the_fp32_spec_gives():
    g = es.graph("bip.txt")
    field, _n = es.load_fields(g, "bip_field.txt")
    ev = es.q_eval_records(g, field)
    W0, _I0 = es.glibc_tables(g.V, es.Q_DIM)
    assert abs(es.loss(W0.astype(np.float32).astype(np.float64), es.Q_K, ev) - es.Q_UNTRAINED) < 5e-5
    for seed, want in zip(es.Q_SEEDS, es.Q_SPEC):
        W = es.padded(W0.astype(np.float32), es.Q_DIM)
        es.run(g, field, W, es.Q_K, es.Q_ALPHA, es.Q_REG, es.Q_SAMPLES, 0, es.Q_SAMPLES, seed)
        assert abs(es.loss(W[:, :es.Q_DIM].astype(np.float64), es.Q_K, ev) - want) < 5e-5
    # the objective has fallen by far more than the bar's margin at Q_SAMPLES samples
    assert es.Q_UNTRAINED - max(es.Q_SPEC) > 10 * (es.q_bar() - max(es.Q_SPEC))


def test_generated_graph_offers_clean_and_ordered_samples():
    """What test_gpu_eco.py's together-path test relies on, checked without a GPU."""
    from smore_amd import graphgen
    g, field, _e = es.load_graph(graphgen.bipartite_edges(es.LOAD_USERS, es.LOAD_ITEMS, es.LOAD_LINES, es.LOAD_SEED))
    for K in (5, 20):
        r = es.run(g, field, None, K, 0.025, 0.01, 10 ** 6, 0, 3000, 20251015)
        assert r.skipped == 0 and (r.clean == 1).sum() > 1000 and (r.clean == 0).sum() >= 1
