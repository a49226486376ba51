"""HOP-REC on the CPU: the field loader of the library (host-only context),
the rule's spec (tests/c/hoprec_spec.c) against the reference's own runs
(tests/golden/updates_hoprec.npz, e2e_hoprec_bip.npz; how they were made:
DESIGN.md 6 and 12b), the conditions the committed trials must meet, and
where the fp32 and the fp64 instance of the rule part ways."""
import os

import numpy as np
import pytest

from tests import hoprec_spec as hs
from tests.conftest import GOLDEN

TOTAL, TAGS, Trials, gold = hs.TOTAL, hs.TAGS, hs.Trials, hs.gold


@pytest.fixture(scope="module")
def fixtures():
    z = gold("updates_hoprec")
    return {tag: Trials(z, tag) for tag in TAGS}


def test_lib_binding_declares_hoprec():
    from smore_amd import _lib
    sig = _lib.lib._signatures
    assert sig["smore_train_hoprec"] == sig["smore_train_hoprec_async"]
    assert len(sig["smore_train_hoprec"][1]) == 8 and len(sig["smore_hoprec_stats"][1]) == 3
    assert len(sig["smore_hoprec_records"][1]) == 7
    for name in ("smore_load_field_meta", "smore_field_meta_info", "smore_set_fields", "smore_get_fields"):
        assert name in sig
    import smore_amd
    assert "HBPR" in smore_amd.__all__
    for m in ("LoadFieldMeta", "set_fields", "fields", "train_hoprec", "hoprec_stats", "hoprec_records"):
        assert hasattr(smore_amd.ProNet, m)


# ---------------------------------------------------------------- the field loader (host-only)
def host_pronet(fname, undirected=1):
    import smore_amd
    pn = smore_amd.ProNet(-1)
    pn.SetNegativeMethod("no_degrees")
    pn.LoadEdgeList(os.path.join(GOLDEN, fname), undirected)
    return pn


@pytest.mark.parametrize("gfile,ffile,nf", [("bip.txt", "bip_field.txt", 2), ("toy.txt", "toy_field.txt", 2),
                                            ("pl100w.txt", "pl100w_field3.txt", 3)])
def test_field_loader_matches_the_reference_rule(gfile, ffile, nf):
    pn = host_pronet(gfile)
    assert pn.fields == (None, 0)
    pn.LoadFieldMeta(os.path.join(GOLDEN, ffile))
    field, n = pn.fields
    g = hs.graph(gfile)
    want, wn = hs.load_fields(g, ffile)
    assert n == wn == nf and pn.names == g.names
    np.testing.assert_array_equal(field, want)
    if gfile == "bip.txt":   # the reference's own LoadFieldMeta, dumped with the e2e run
        np.testing.assert_array_equal(field, gold("e2e_hoprec_bip")["field"])
        assert all((f == 0) == name.startswith("u") for f, name in zip(field, g.names))
    if gfile == "pl100w.txt":
        assert all(f == int(name[1:]) % 3 for f, name in zip(field, g.names))


def test_field_ids_by_first_appearance_absent_and_unknown(tmp_path):
    pn = host_pronet("toy.txt")
    names = pn.names
    p = tmp_path / "f.txt"
    # the first field named is field 0 whatever it is called; a name outside the graph
    # is passed over but its field still takes the next id (src/proNet.cpp:368-377)
    p.write_text("%s zeta\nnobody alpha\n%s beta\n%s zeta\n" % (names[1], names[2], names[3]))
    assert pn.LoadFieldMeta(str(p)) == (4, 1)   # lines read, names passed over: reported
    field, n = pn.fields
    assert n == 3
    want = np.zeros(len(names), np.int32)   # vertices the file does not name keep field 0
    want[2] = 2
    np.testing.assert_array_equal(field, want)
    # a new graph drops the fields
    pn.LoadEdgeList(os.path.join(GOLDEN, "toy.txt"), 1)
    assert pn.fields == (None, 0)


def test_set_fields_range_checks():
    from smore_amd import _lib
    pn = host_pronet("toy.txt")
    V = pn.MAX_vid
    f = np.arange(V, dtype=np.int32) % 2
    pn.set_fields(f, 2)
    got, n = pn.fields
    assert n == 2
    np.testing.assert_array_equal(got, f)
    for bad, nf in ((np.full(V, 2, np.int32), 2), (np.full(V, -1, np.int32), 2), (f, 0)):
        with pytest.raises(_lib.SmoreError):
            pn.set_fields(bad, nf)
    with pytest.raises(ValueError):
        pn.set_fields(f[:-1], 2)
    np.testing.assert_array_equal(pn.fields[0], f)   # a refused call leaves the fields


# ---------------------------------------------------------------- fp64 spec vs the reference
@pytest.mark.parametrize("tag", TAGS)
def test_fp64_spec_reproduces_single_samples_bit_exact(fixtures, tag):
    F = fixtures[tag]
    if tag != "bip64":
        assert np.array_equal(F.z[tag + "_W0"], hs.lcg_table(F.g.V, F.dim))
    assert F.z[tag + "_others_unchanged"].all()
    for t in range(F.n):
        s, slots, _kind, _rej, rec, pbits, T0, want = F.trial(t)
        T = T0.copy()
        r = F.run(T, s)
        assert r.skipped == 0
        np.testing.assert_array_equal(r.rec[0, :F.nw], rec)
        assert (r.rec[0, F.nw:] == -1).all()
        assert r.slots[0] == slots
        np.testing.assert_array_equal(r.passed[0], pbits)
        assert (r.tested, r.npassed) == (5 * F.steps, int(pbits.sum()))
        # the touched rows, and every other row unchanged
        assert np.array_equal(T, want), (tag, t)


def test_fp64_spec_reproduces_end_to_end_bit_exact():
    z = gold("e2e_hoprec_bip")
    dim, st, steps, seed = (int(x) for x in z["meta"])
    g = hs.graph("bip.txt")
    T = z["W0"].copy()
    r = hs.run(g, z["field"], T, steps, float(z["meta_f"][0]), st * 10 ** 6, 0, st * 10 ** 6, seed)
    assert r.skipped == 0
    assert np.array_equal(T, z["W"])


def test_committed_trials_meet_their_conditions(fixtures):
    plain = closed_gate = mixed = rejected = nclosed = 0
    eij = evj = 0
    for tag, F in fixtures.items():
        for t in range(F.n):
            s, _slots, kind, rej, rec, pbits, T0, want = F.trial(t)
            rejected += rej
            if kind:   # closed gates: nothing changes
                nclosed += tag.startswith("bip")
                assert not pbits.any() and np.array_equal(T0, want)
                T = T0.copy()
                r = F.run(T, s)
                assert (r.tested, r.npassed) == (5 * F.steps, 0) and np.array_equal(T, T0)
                pos = {int(rec[0])} | {int(rec[1 + 6 * w]) for w in range(F.steps)}
                assert not pos & {int(rec[2 + 6 * w + k]) for w in range(F.steps) for k in range(5)}
                continue
            plain += 1
            closed_gate += not pbits.all()
            up = pbits.sum(1)
            mixed += bool((up == 0).any() and (up > 0).any())
            if tag == "pl3":
                for w in range(F.steps):
                    js = rec[2 + 6 * w:7 + 6 * w]
                    eij += int((js == rec[1 + 6 * w]).any())
                    evj += int((js == rec[0]).any())
    assert closed_gate >= 0.5 * plain, (closed_gate, plain)
    assert mixed >= 1 and eij >= 1 and evj >= 1 and rejected >= 1 and nclosed >= 3


def test_margins_of_committed_trials(fixtures):
    """The GPU comparison with the reference leaves out trials in which any
    gate's fp64 |f - margin_w| is below 1e-4: at most 5 % of the committed
    trials may be such."""
    small = total = 0
    for F in fixtures.values():
        for t in range(F.n):
            s, *_rest, T0, _want = F.trial(t)
            small += F.run(T0.copy(), s).margin < 1e-4
            total += 1
    assert small <= 0.05 * total, (small, total)


@pytest.mark.parametrize("tag", TAGS)
def test_fp32_spec_single_samples_within_1e5(fixtures, tag):
    """The fp32 instance against the reference on one sample (the bar of the
    other rules' single-sample parity), trials with a margin >= 1e-4."""
    F = fixtures[tag]
    for t in range(F.n):
        s, _slots, _kind, _rej, _rec, pbits, T0, want = F.trial(t)
        if F.run(T0.copy(), s).margin < 1e-4:
            continue
        T32 = hs.padded(T0.astype(np.float32), F.dim)
        r = F.run(T32, s)
        np.testing.assert_array_equal(r.passed[0], pbits)
        np.testing.assert_allclose(T32[:, :F.dim], want, atol=1e-5, rtol=0)
        assert not T32[:, F.dim:].any()


def test_recorded_spec_auc_is_what_the_fp32_spec_gives():
    """The GPU scatter test's bar (test_gpu_hoprec.py) is derived from
    hoprec_spec.SPEC_AUC: the fp32 spec's AUC on bip.txt at three seeds."""
    g = hs.graph("bip.txt")
    field, _n = hs.load_fields(g, "bip_field.txt")
    W0 = hs.glibc_table(g.V, hs.AUC_DIM)
    for seed, want in zip(hs.AUC_SEEDS, hs.SPEC_AUC):
        T = hs.padded(W0, hs.AUC_DIM)
        hs.run(g, field, T, hs.AUC_STEPS, 0.025, hs.AUC_SAMPLES, 0, hs.AUC_SAMPLES, seed)
        assert abs(hs.auc(g, field, T[:, :hs.AUC_DIM]) - want) < 5e-5, seed


def test_branch_divergence_of_fp32_and_fp64_is_a_margin_decision():
    """Whole run, fp32 against fp64 (the WARP treatment).  If the two
    instances' pass bits differ anywhere on the 10^6-sample run, then up to the
    first sample that differs they took the same branches, and at that sample
    the first differing gate's fp64 margin |f - margin_w| is within the bound
    on |f32 - f64| that the tables' difference at that point allows: the split
    is a rounding decision, not a rule bug.  The end distance is measured and
    printed, not asserted."""
    z = gold("e2e_hoprec_bip")
    dim, st, steps, seed = (int(x) for x in z["meta"])
    alpha, total = float(z["meta_f"][0]), st * 10 ** 6
    g, field = hs.graph("bip.txt"), z["field"]
    A, B = z["W0"].copy(), hs.padded(z["W0"].astype(np.float32), dim)
    p64 = hs.run(g, field, A, steps, alpha, total, 0, total, seed).passed
    p32 = hs.run(g, field, B, steps, alpha, total, 0, total, seed).passed
    print("end distance max|spec32 - reference| = %.3e" % np.abs(B[:, :dim] - z["W"]).max())
    diff = np.nonzero((p64 != p32).reshape(total, -1).any(1))[0]
    print("samples whose pass bits differ: %d, first %s" % (len(diff), diff[:1]))
    if len(diff) == 0:
        return   # full agreement: nothing to bound
    s = int(diff[0])
    A, B = z["W0"].copy(), hs.padded(z["W0"].astype(np.float32), dim)
    hs.run(g, field, A, steps, alpha, total, 0, s, seed)
    hs.run(g, field, B, steps, alpha, total, 0, s, seed)
    # the first differing gate of sample s: step w, negative n
    w, n = (int(x) for x in np.argwhere(p64[s] != p32[s])[0])
    # sample s up to that gate in both instances: the tables as the gate finds them
    f64 = hs.run(g, field, A, steps, alpha, total, s, s + 1, seed, stop=5 * w + n)
    f32 = hs.run(g, field, B, steps, alpha, total, s, s + 1, seed, stop=5 * w + n)
    delta = np.abs(A - B[:, :dim]).max()
    big = max(np.abs(A).max(), np.abs(B).max())
    # f = sum_k wv_k (wi_k - wj_k): |df| <= d (delta * 2 big + big * 2 delta), plus the
    # fp32 evaluation's own rounding, d + 2 operations of relative 2^-24 on terms <= 2 big^2
    bound = dim * 4 * delta * big + (dim + 2) * 2.0 ** -24 * dim * 2 * big * big
    m64 = abs(f64 - 1.0 / (w + 1))
    print("first split: sample %d step %d negative %d  f64 %.9g f32 %.9g  margin %.3e bound %.3e"
          % (s, w + 1, n, f64, f32, m64, bound))
    assert (f64 > 1.0 / (w + 1)) != (f32 > np.float32(1.0 / (w + 1)))   # it is this gate that splits
    assert m64 <= bound, (s, w, n, m64, bound, delta)

