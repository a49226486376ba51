"""The set-sum (CBOW) rule of GCN and TEXTGCN on the CPU: the spec (tests/c/cbow_spec.c)
against the reference's own runs (tests/golden/updates_cbow.npz, e2e_gcn_bip.npz,
e2e_textgcn_pl.npz), and the interface's names.

  * fp64 spec vs every single-sample trial   : bit for bit (record, slots, buckets, rows)
  * fp64 spec vs both 10^6-sample runs       : bit for bit
  * fp32 spec vs the trials                  : 1e-5 where the sigmoid buckets agree (<= 5 % may not)
  * the spec-level writer                    : the reference's saved bytes
"""
import numpy as np
import pytest

from tests import cbow_spec as cs

GCN, TEXTGCN = cs.GCN, cs.TEXTGCN


def test_interface_names():
    import smore_amd
    from smore_amd import _lib
    sig = _lib.lib._signatures
    assert sig["smore_train_cbow"] == sig["smore_train_cbow_async"]
    assert len(sig["smore_train_cbow"][1]) == 11 and len(sig["smore_cbow_stats"][1]) == 3
    assert len(sig["smore_cbow_records"][1]) == 9 and len(sig["smore_save_weights_textgcn"][1]) == 3
    for m in ("train_cbow", "cbow_stats", "cbow_records", "save_weights_textgcn"):
        assert callable(getattr(smore_amd.ProNet, m))
    for cls in ("GCN", "TEXTGCN"):
        assert cls in smore_amd.__all__
        for m in ("LoadEdgeList", "LoadFieldMeta", "Init", "Train", "SaveWeights"):
            assert callable(getattr(getattr(smore_amd, cls), m))


@pytest.fixture(scope="module")
def fixtures():
    return cs.all_trials()


def test_fp64_spec_reproduces_every_trial_bit_for_bit(fixtures):
    n = 0
    for F in fixtures.values():
        assert int(F.z[F.key + "_others_unchanged"][0]) == 1
        for t in range(F.n):
            s, slots, rec, bucket, T0, want = F.trial(t)
            W = T0.copy()
            r = F.run(W, s)
            np.testing.assert_array_equal(r.rec[0], rec, err_msg="%s %d" % (F.key, t))
            assert (r.slots[0], r.used[0], r.skipped) == (slots, slots, 0)
            np.testing.assert_array_equal(r.bucket[0], bucket)
            assert W.tobytes() == want.tobytes(), (F.key, t)   # the touched rows, every other row unchanged
            assert r.clean[0] == cs.is_clean(rec, F.S, F.K)
            n += 1
    assert n == 112


def test_committed_trials_cover_the_cases(fixtures):
    n = clean = 0
    seen = dict(dup_c=0, dup_neg=0, neg_in_c=0, neg_in_earlier_neg=0, w_in_c=0, w_in_neg=0, empty=0)
    for F in fixtures.values():
        for t in range(F.n):
            rec = F.trial(t)[2]
            c, w, neg = cs.sets_of(rec, F.S, F.K)
            flat = [x for s in neg for x in s]
            n += 1
            clean += cs.is_clean(rec, F.S, F.K)
            seen["dup_c"] += len(set(c)) < len(c)
            seen["dup_neg"] += any(len(set(s)) < len(s) for s in neg)
            seen["neg_in_c"] += bool(set(flat) & set(c))
            seen["neg_in_earlier_neg"] += any(set(neg[k]) & {x for s in neg[:k] for x in s} for k in range(1, len(neg)))
            seen["w_in_c"] += bool(set(w) & set(c))
            seen["w_in_neg"] += bool(set(w) & set(flat))
            seen["empty"] += not w or not c   # the directed toy load: an item has no out-edge
    print("trials %d, clean %d, %s" % (n, clean, seen))
    assert clean >= 0.25 * n
    assert all(v >= 1 for v in seen.values()), seen


def test_fp32_spec_within_1e5_of_the_reference(fixtures):
    left, n, worst = [], 0, 0.0
    for F in fixtures.values():
        for t in range(F.n):
            s, _slots, _rec, bucket, T0, want = F.trial(t)
            n += 1
            W = cs.padded(T0.astype(np.float32), F.dim)
            r = F.run(W, s)
            if not np.array_equal(r.bucket[0], bucket):
                left.append((F.key, t))   # an fp32 dot fell into another sigmoid bucket
                continue
            assert (W[:, F.dim:] == 0).all()
            worst = max(worst, float(np.abs(W[:, :F.dim] - want).max()))
            np.testing.assert_allclose(W[:, :F.dim], want, atol=1e-5, rtol=0, err_msg="%s %d" % (F.key, t))
    print("left out (another sigmoid bucket): %s of %d; worst |fp32 - reference| %.3g" % (left, n, worst))
    assert len(left) <= 0.05 * n


@pytest.fixture(scope="module")
def whole_runs():
    out = {}
    for model in (GCN, TEXTGCN):
        name, gf, ff = cs.E2E[model]
        z = cs.gold(name)
        g = cs.graph(gf)
        field, _n = cs.load_fields(g, ff)
        dim, st, S, K, seed = (int(x) for x in z["meta"])
        alpha, reg = (float(x) for x in z["meta_f"])
        W = z["W0"].copy()
        r = cs.run(g, field, W, model, S, K, alpha, reg, st * 10 ** 6, 0, st * 10 ** 6, seed)
        W32 = cs.padded(z["W0"].astype(np.float32), dim)
        cs.run(g, field, W32, model, S, K, alpha, reg, st * 10 ** 6, 0, st * 10 ** 6, seed)
        out[model] = (z, g, field, W, W32[:, :dim], r)
    return out


@pytest.mark.parametrize("model", [GCN, TEXTGCN])
def test_fp64_spec_reproduces_the_whole_run(whole_runs, model):
    z, g, field, W, W32, r = whole_runs[model]
    np.testing.assert_array_equal(field, z["field"])
    W0, C0 = cs.glibc_tables(g.V, W.shape[1])   # Init: w_vertex, then w_context, one rand() stream
    assert W0.tobytes() == z["W0"].tobytes() and C0.tobytes() == z["C0"].tobytes()
    assert r.skipped == 0
    assert W.tobytes() == z["W"].tobytes()
    # fp32 against fp64 over the whole run: measured, no bar
    print("%s: max |spec32 - reference| = %.3g (max |reference| %.3g), clean samples %d of 10^6"
          % (cs.MODELS[model], np.abs(W32 - z["W"]).max(), np.abs(z["W"]).max(), int((r.clean == 1).sum())))
    assert np.isfinite(W32).all()


@pytest.mark.parametrize("model", [GCN, TEXTGCN])
def test_spec_writer_reproduces_the_saved_file(whole_runs, model):
    z, g, field, _W, _W32, _r = whole_runs[model]
    text = cs.save_lines(g, field, model, z["W"], z["C0"])
    assert text == z["saved"].tobytes()
    lines = text.decode().splitlines()
    if model == TEXTGCN:   # field-1 vertices are left out, field 0 writes a sum, field 2 its own row
        assert int(lines[0].split()[0]) == int((field != 1).sum()) == len(lines) - 1 < g.V
        assert set(np.unique(field)) == {0, 1, 2}
    else:
        assert int(lines[0].split()[0]) == g.V == len(lines) - 1


@pytest.mark.parametrize("model", [GCN, TEXTGCN])
def test_recorded_spec_objective_is_what_the_fp32_spec_gives(model):
    g = cs.graph("bip.txt")
    field, _n = cs.load_fields(g, "bip_field.txt")
    ev = cs.q_eval_records(g, field, model)
    W0, _C0 = cs.glibc_tables(g.V, cs.Q_DIM)
    assert abs(cs.loss(W0, cs.Q_S, cs.Q_K, ev) - cs.Q_UNTRAINED[model]) < 5e-5
    for seed, want in zip(cs.Q_SEEDS, cs.Q_SPEC[model]):
        W = cs.padded(W0.astype(np.float32), cs.Q_DIM)
        cs.run(g, field, W, model, cs.Q_S, cs.Q_K, cs.Q_ALPHA, cs.Q_REG, cs.Q_SAMPLES, 0, cs.Q_SAMPLES, seed)
        assert abs(cs.loss(W[:, :cs.Q_DIM].astype(np.float64), cs.Q_S, cs.Q_K, ev) - want) < 5e-5
    # the objective has fallen by far more than the bar's margin at Q_SAMPLES samples
    assert cs.Q_UNTRAINED[model] - max(cs.Q_SPEC[model]) > 10 * (cs.q_bar(model) - max(cs.Q_SPEC[model]))


def test_generated_graph_offers_clean_and_ordered_samples():
    """What test_gpu_cbow.py's together-path test relies on, checked without a GPU."""
    from smore_amd import graphgen
    g, field, _e = cs.load_graph(graphgen.bipartite_edges(cs.LOAD_USERS, cs.LOAD_ITEMS, cs.LOAD_LINES, cs.LOAD_SEED))
    for model in (GCN, TEXTGCN):
        r = cs.run(g, field, None, model, 5, 5, 0.025, 0.01, 10 ** 6, 0, 3000, 20251015)
        assert r.skipped == 0 and (r.clean == 1).sum() > 1500 and (r.clean == 0).sum() >= 1
