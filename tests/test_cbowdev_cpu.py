"""The bag-of-words event rule of TEXTGCNdev on the CPU: the spec (tests/c/cbowdev_spec.c)
against the reference's own runs (tests/golden/updates_cbowdev.npz, e2e_textgcndev_pl.npz),
and the interface's names.

  * fp64 spec vs every single-sample trial   : bit for bit (record, slots, buckets, rows)
  * fp64 spec vs the 10^6-sample run         : bit for bit, both tables
  * fp32 spec vs the trials                  : 1e-5 where the sigmoid buckets agree (<= 5 % may not)
  * the spec-level writer                    : the reference's saved bytes
  * the reference's accidents                : the last event's rows move; label 0 from iteration 1 on
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import cbowdev_spec as cs


def test_interface_names():
    import smore_amd
    from smore_amd import _lib
    sig = _lib.lib._signatures
    assert sig["smore_train_cbowdev"] == sig["smore_train_cbowdev_async"]
    assert len(sig["smore_train_cbowdev"][1]) == 10 and len(sig["smore_cbowdev_stats"][1]) == 3
    assert len(sig["smore_cbowdev_records"][1]) == 8 and len(sig["smore_save_weights_textgcndev"][1]) == 3
    for m in ("train_cbowdev", "cbowdev_stats", "cbowdev_records", "save_weights_textgcndev"):
        assert callable(getattr(smore_amd.ProNet, m))
    assert "TEXTGCNdev" in smore_amd.__all__
    for m in ("LoadEdgeList", "LoadFieldMeta", "Init", "Train", "SaveWeights"):
        assert callable(getattr(smore_amd.TEXTGCNdev, m))


@pytest.fixture(scope="module")
def fixtures():
    return cs.all_trials()


def test_fp64_spec_reproduces_every_trial_bit_for_bit(fixtures):
    n = skips = 0
    for F in fixtures.values():
        # per trial: in the reference's own run no row the record does not name changed, in either table
        assert F.z[F.key + "_others_unchanged"].shape == (F.n,) and (F.z[F.key + "_others_unchanged"] == 1).all()
        for t in range(F.n):
            s, slots, rec, bucket, W, Cx = F.trial(t)
            a, b = F.W0.copy(), F.C0.copy()
            r = F.run(a, b, s)
            np.testing.assert_array_equal(r.rec[0], rec, err_msg="%s %d" % (F.key, t))
            skip = int(rec[0] < 0)
            assert (r.slots[0], r.used[0], r.skipped) == (slots, slots, skip)
            np.testing.assert_array_equal(r.bucket[0], bucket)
            assert a.tobytes() == W.tobytes() and b.tobytes() == Cx.tobytes(), (F.key, t)   # every other row unchanged
            assert r.clean[0] == (-1 if skip else cs.is_clean(rec, F.E, F.N))
            np.testing.assert_array_equal(cs.events_of(F.g, F.field, F.seed, s, F.E, F.N), F.z[F.key + "_events"][t])
            n += 1
            skips += skip
    assert (n, skips) == (127, 20)


def test_committed_trials_cover_the_cases(fixtures):
    seen = {cs.CASE_CLEAN: 0, cs.CASE_NEG_IS_EVENT: 0, cs.CASE_REPEATED_NEG: 0, cs.CASE_REPEATED_BAG: 0,
            cs.CASE_EVENTS_DIFFER: 0}
    for F in fixtures.values():
        for t in range(F.n):
            rec, ev = F.z[F.key + "_rec"][t], F.z[F.key + "_events"][t]
            if rec[0] < 0:
                assert not F.undirected and (rec == -1).all()   # the directed toy load: an item has no out-edge
                continue
            neg = [int(x) for x in rec[2 + F.E * F.N:F.nw]]
            bag = [int(x) for x in rec[2:2 + F.E * F.N]]
            got = (cs.CASE_CLEAN * cs.is_clean(rec, F.E, F.N) | cs.CASE_NEG_IS_EVENT * (int(rec[1]) in neg)
                   | cs.CASE_REPEATED_NEG * (len(set(neg)) < len(neg)) | cs.CASE_REPEATED_BAG * (len(set(bag)) < len(bag))
                   | cs.CASE_EVENTS_DIFFER * bool((ev != rec[1]).any()))
            assert got == int(F.z[F.key + "_cases"][t])
            for k in seen:
                seen[k] += bool(got & k)
    print(seen)
    assert all(v >= 1 for v in seen.values()), seen


def test_fp32_spec_within_1e5_of_the_reference(fixtures):
    left, n, worst = [], 0, 0.0
    for F in fixtures.values():
        for t in range(F.n):
            s, _slots, _rec, bucket, W, Cx = F.trial(t)
            n += 1
            a, b = cs.padded(F.W0.astype(np.float32), F.dim), cs.padded(F.C0.astype(np.float32), F.dim)
            r = F.run(a, b, s)
            if not np.array_equal(r.bucket[0], bucket):
                left.append((F.key, t))   # an fp32 dot fell into another sigmoid bucket
                continue
            assert (a[:, F.dim:] == 0).all() and (b[:, F.dim:] == 0).all()
            worst = max(worst, float(np.abs(a[:, :F.dim] - W).max()), float(np.abs(b[:, :F.dim] - Cx).max()))
            np.testing.assert_allclose(a[:, :F.dim], W, atol=1e-5, rtol=0, err_msg="%s %d" % (F.key, t))
            np.testing.assert_allclose(b[:, :F.dim], Cx, atol=1e-5, rtol=0, err_msg="%s %d" % (F.key, t))
    print("left out (another sigmoid bucket): %s of %d; worst |fp32 - reference| %.3g" % (left, n, worst))
    assert len(left) <= 0.05 * n


# ---------------------------------------------------------------- the accidents, from the fixtures
def test_accident_the_rows_moved_are_the_last_events(fixtures):
    """The update loop uses the variable the collection loop left behind: with events e0 != e_last,
    W[e_last] moves and W[e0] does not (unless a negative names it), while both events' words
    are in the bag."""
    n = 0
    for F in fixtures.values():
        for t in range(F.n):
            rec, ev = F.z[F.key + "_rec"][t], F.z[F.key + "_events"][t]
            if F.E < 2 or rec[0] < 0 or (ev == ev[-1]).all():
                continue
            assert rec[1] == ev[-1]
            _s, _slots, _rec, _bucket, W, _Cx = F.trial(t)
            assert not np.array_equal(W[ev[-1]], F.W0[ev[-1]])
            neg = set(int(x) for x in rec[2 + F.E * F.N:F.nw])
            for e in ev[:-1]:
                if e != ev[-1] and int(e) not in neg and e != rec[0]:
                    assert W[e].tobytes() == F.W0[e].tobytes()   # recorded unchanged by the reference run
                    n += 1
    assert n >= 1


def _step(row, ctx, label, alpha, reg):
    """Opt_SigmoidRegSGD on the row as its own loss vector, in numpy fp64: (bucket, updated row)."""
    f = 0.0
    for k in range(len(row)):
        f += float(row[k]) * float(ctx[k])
    g = label - orc.fast_sigmoid(f)
    return int((f + 8.0) * 1000 / 8.0 / 2), row + alpha * (g * ctx - reg * row)


def test_accident_only_iteration_0_has_label_1(fixtures):
    """label is set to 1 before the loop and to 0 inside it: from iteration 1 on the two steps on
    W[event] run with label 0.  The event row is followed by hand through its 2 E steps."""
    n = 0
    for F in fixtures.values():
        for t in range(F.n):
            rec = F.z[F.key + "_rec"][t]
            if F.E < 2 or rec[0] < 0 or rec[1] == rec[0] or int(rec[1]) in [int(x) for x in rec[2 + F.E * F.N:F.nw]]:
                continue
            bucket, want = F.z[F.key + "_bucket"][t], F.z[F.key + "_rows"][t][1]
            w_avg = np.zeros(F.dim)
            for v in rec[2:2 + F.E * F.N]:
                w_avg = w_avg + F.C0[v]
            rows = {}
            for later in (0.0, 1.0):
                row = F.W0[rec[1]].copy()
                for i in range(F.E):
                    label = 1.0 if i == 0 else later
                    b0, row = _step(row, w_avg, label, F.alpha, F.reg)
                    b1, row = _step(row, F.W0[rec[0]], label, F.alpha, F.reg)
                    if later == 0.0:
                        assert (b0, b1) == (int(bucket[12 * i]), int(bucket[12 * i + 1])), (F.key, t, i)
                rows[later] = row
            assert rows[0.0].tobytes() == want.tobytes(), (F.key, t)
            assert rows[1.0].tobytes() != want.tobytes()
            n += 1
    assert n >= 3


# ---------------------------------------------------------------- the whole run
@pytest.fixture(scope="module")
def whole_run():
    name, gf, ff = cs.E2E
    z = cs.gold(name)
    g = cs.graph(gf)
    field, _n = cs.load_fields(g, ff)
    dim, st, E, N, seed = (int(x) for x in z["meta"])
    alpha, reg = (float(x) for x in z["meta_f"])
    W, Cx = z["W0"].copy(), z["C0"].copy()
    r = cs.run(g, field, W, Cx, E, N, alpha, reg, st * 10 ** 6, 0, st * 10 ** 6, seed)
    W32, C32 = cs.padded(z["W0"].astype(np.float32), dim), cs.padded(z["C0"].astype(np.float32), dim)
    cs.run(g, field, W32, C32, E, N, alpha, reg, st * 10 ** 6, 0, st * 10 ** 6, seed)
    return z, g, field, W, Cx, W32[:, :dim], C32[:, :dim], r


def test_fp64_spec_reproduces_the_whole_run(whole_run):
    z, g, field, W, Cx, W32, C32, r = whole_run
    np.testing.assert_array_equal(field, z["field"])
    assert tuple(int(x) for x in z["meta"][1:4]) == (1, 1, 5) and tuple(z["meta_f"]) == (0.025, 0.01)   # the CLI defaults
    W0, C0 = cs.glibc_tables(g.V, W.shape[1])   # Init: w_vertex whole, then w_context, one rand() stream
    assert W0.tobytes() == z["W0"].tobytes() and C0.tobytes() == z["C0"].tobytes()
    assert r.skipped == 0
    assert W.tobytes() == z["W"].tobytes() and Cx.tobytes() == z["C"].tobytes()
    assert np.isfinite(z["W"]).all() and np.isfinite(z["C"]).all()   # the reference's run is finite at alpha 0.025
    # fp32 against fp64 over the whole run: measured (2.2e-4 on W, 9.7e-5 on C).  It
    # is above 1e-4, so class and CLI are held to the fp32 spec (test_gpu_cbowdev.py)
    gap = max(float(np.abs(W32 - z["W"]).max()), float(np.abs(C32 - z["C"]).max()))
    print("max |spec32 - reference| = %.3g (max |reference| %.3g), clean samples %d of 10^6"
          % (gap, max(np.abs(z["W"]).max(), np.abs(z["C"]).max()), int((r.clean == 1).sum())))
    assert np.isfinite(W32).all() and np.isfinite(C32).all()
    assert 1e-4 < gap < 1e-2


def test_spec_writer_reproduces_the_saved_file(whole_run):
    z, g, field, _W, _Cx, _W32, _C32, _r = whole_run
    text = cs.save_lines(g, field, z["W"], z["C"])
    assert text == z["saved"].tobytes()
    lines = text.decode().splitlines()
    # field-1 vertices are left out, field 0 writes its w_vertex row, field 2 its w_context row
    assert int(lines[0].split()[0]) == int((field != 1).sum()) == len(lines) - 1 < g.V
    assert set(np.unique(field)) == {0, 1, 2}
    assert all(len(ln.split()) == 1 + z["W"].shape[1] for ln in lines[1:])


def test_recorded_spec_objective_is_what_the_fp32_spec_gives():
    g = cs.graph("bip.txt")
    field, _n = cs.load_fields(g, "bip_field.txt")
    ev = cs.q_eval_records(g, field)
    W0, C0 = cs.glibc_tables(g.V, cs.Q_DIM)
    assert abs(cs.loss(W0, C0, cs.Q_E, cs.Q_N, ev) - cs.Q_UNTRAINED) < 5e-5
    for seed, want in zip(cs.Q_SEEDS, cs.Q_SPEC):
        W, Cx = cs.padded(W0.astype(np.float32), cs.Q_DIM), cs.padded(C0.astype(np.float32), cs.Q_DIM)
        cs.run(g, field, W, Cx, cs.Q_E, cs.Q_N, cs.Q_ALPHA, cs.Q_REG, cs.Q_SAMPLES, 0, cs.Q_SAMPLES, seed)
        q = cs.loss(W[:, :cs.Q_DIM].astype(np.float64), Cx[:, :cs.Q_DIM].astype(np.float64), cs.Q_E, cs.Q_N, ev)
        assert abs(q - want) < 5e-5
    # the objective has fallen by far more than the bar's margin at Q_SAMPLES samples
    assert cs.Q_UNTRAINED - max(cs.Q_SPEC) > 10 * (cs.q_bar() - max(cs.Q_SPEC))


def test_generated_graph_populates_both_paths():
    """What test_gpu_cbowdev.py's load test relies on, checked without a GPU: at (3, 2), 32 row ids
    per sample among 2^14 items, at least 10 % of the samples are clean and at least 1 % ordered
    (at (1, 5), 12 ids, only 0.2 % would be ordered)."""
    from smore_amd import graphgen
    g, field, _e = cs.load_graph(graphgen.bipartite_edges(cs.LOAD_USERS, cs.LOAD_ITEMS, cs.LOAD_LINES, cs.LOAD_SEED))
    r = cs.run(g, field, None, None, 3, 2, 0.025, 0.01, 10 ** 6, 0, 3000, 20251015)
    assert r.skipped == 0 and (r.clean == 1).sum() >= 300 and (r.clean == 0).sum() >= 30


def test_ten_by_ten_diverges_at_the_default_alpha():
    """Why the GPU parity case (10, 10) runs at alpha 0.005: 120 steps per sample on a bag of 100
    rows blow up at 0.025, in the reference's own arithmetic (fp64) too."""
    g = cs.graph("bip.txt")
    field, _n = cs.load_fields(g, "bip_field.txt")
    sc = (12.0 / 64) ** 0.5
    for alpha, n, ok in ((0.025, 100, False), (0.005, 3000, True)):
        W, Cx = (x * sc for x in cs.start_tables(g.V, 64))
        cs.run(g, field, W, Cx, 10, 10, alpha, 0.01, 10 ** 6, 9000, 9000 + n, 20251015)
        assert (max(np.abs(W).max(), np.abs(Cx).max()) < 10) == ok
