"""HOP-REC on the GPU (smore_train_hoprec, smore_hoprec_records,
smore_amd.HBPR, bin/hoprec) against the rule's CPU spec
(tests/c/hoprec_spec.c) and the reference's own runs
(tests/golden/updates_hoprec.npz).  Needs an MI355X.

  * the draw kernel's records and slot counts  : equal to the spec's
  * serial mode vs the fp32 spec               : bit-exact, counters included
  * one sample vs the reference (fp64)         : 1e-5 absolute, margins >= 1e-4
  * closed gates                               : table bytes unchanged
  * atomic / hybrid scatter                    : ranking AUC of the CPU fp32 spec
  * 10^6-sample run vs the reference           : NOT compared -- the fp32 and
    fp64 runs part ways at a margin decision (test_hoprec_cpu.py, DESIGN.md
    12b); the model class and the CLI are held to the fp32 spec of the same
    run instead
"""
import os
import subprocess

import numpy as np
import pytest

from tests import hoprec_spec as hs
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SEED = 20251015
TOTAL, TAGS, Trials, gold = hs.TOTAL, hs.TAGS, hs.Trials, hs.gold
BIN = os.path.join(ROOT, "smore_amd", "bin")
GRAPHS = {"bip": ("bip.txt", "bip_field.txt"), "toy": ("toy.txt", "toy_field.txt"),
          "pl3": ("pl100w.txt", "pl100w_field3.txt")}


@pytest.fixture(scope="module")
def smore():
    import smore_amd
    return smore_amd


def make_pair(smore, key):
    gfile, ffile = GRAPHS[key]
    g = hs.graph(gfile)
    field, _n = hs.load_fields(g, ffile)
    pn = smore.ProNet(0)
    pn.SetNegativeMethod("no_degrees")
    pn.LoadEdgeList(os.path.join(GOLDEN, gfile), 1)
    pn.LoadFieldMeta(os.path.join(GOLDEN, ffile))
    assert pn.MAX_vid == g.V
    np.testing.assert_array_equal(pn.fields[0], field)
    return g, field, pn


# ---------------------------------------------------------------- the draws
@pytest.mark.parametrize("key", ["bip", "pl3"])
@pytest.mark.parametrize("steps", [1, 5, 10])
def test_records_equal_the_spec(smore, key, steps):
    g, field, pn = make_pair(smore, key)
    for begin in (0, (1 << 32) + 12345):   # the second range: a unit counter above 2^32
        n = 20000
        rec, slots = pn.hoprec_records(begin, n, steps, SEED)
        r = hs.run(g, field, None, steps, 0.025, TOTAL, begin, begin + n, SEED)
        assert rec.shape == (n, hs.width(steps))
        np.testing.assert_array_equal(rec, r.rec)
        np.testing.assert_array_equal(slots, r.slots)
        assert r.skipped == 0 and (rec[:, :1 + 6 * steps] >= 0).all()
        assert (field[rec[:, 0]] == 0).all()   # every source is a user
        assert slots.min() >= 10 * steps < slots.max()   # 10 per step without a rejection; rejection loops ran


# ---------------------------------------------------------------- vs the fp32 spec
# d = 5: G = 2 with a padded element; 64 / 128: four / two groups per wave that
# pass different gates; 300: G = 64, two registers per lane, the second chunk
# round partly past dpad; pl3: three fields on 98 vertices, v, i, j coincide
# (the in-order path)
@pytest.mark.parametrize("key,dim,steps", [("toy", 5, 5), ("bip", 5, 5), ("bip", 64, 5), ("bip", 128, 5),
                                           ("bip", 300, 5), ("pl3", 8, 3)])
def test_serial_bit_exact_vs_fp32_spec(smore, key, dim, steps):
    g, field, pn = make_pair(smore, key)
    W0 = hs.lcg_table(g.V, dim).astype(np.float32)
    pn.alloc_tables(dim, 1)
    pn.set_table(0, W0)
    total, begin, n = 10 ** 6, 9000, 3000   # crosses the first alpha step at 10^4
    sk0 = pn.skipped()
    pn.train_hoprec(begin, n, total, steps, 0.05, SEED, "serial")
    W = hs.padded(W0, dim)
    r = hs.run(g, field, W, steps, 0.05, total, begin, begin + n, SEED)
    assert 0 < r.npassed < r.tested == 5 * steps * n   # open and closed gates both
    if key == "pl3":
        rec = r.rec[:, 1:1 + 6 * steps].reshape(n, steps, 6)
        assert (rec[:, :, 1:] == rec[:, :, :1]).any() and (rec[:, :, 1:] == r.rec[:, :1, None]).any()
        assert (rec[:, :, 0] == r.rec[:, :1]).any()   # i == j, v == j and i == v all occur
    np.testing.assert_array_equal(pn.get_table(0), W[:, :dim])
    assert pn.hoprec_stats() == (r.tested, r.npassed)
    assert pn.skipped() - sk0 == r.skipped
    assert pn.last_mode() == "serial"


def test_chunk_independence(smore):
    g, field, pn = make_pair(smore, "bip")
    W0 = hs.lcg_table(g.V, 64).astype(np.float32)
    pn.alloc_tables(64, 1)
    pn.set_table(0, W0)
    pn.train_hoprec(0, 2000, 10 ** 6, 5, 0.05, SEED, "serial")
    one, st_one = pn.get_table(0), pn.hoprec_stats()
    pn.alloc_tables(64, 1)   # zeroes the counters
    assert pn.hoprec_stats() == (0, 0)
    pn.set_table(0, W0)
    pn.train_hoprec(0, 777, 10 ** 6, 5, 0.05, SEED, "serial")
    pn.train_hoprec(777, 2000 - 777, 10 ** 6, 5, 0.05, SEED, "serial")
    np.testing.assert_array_equal(pn.get_table(0), one)
    assert pn.hoprec_stats() == st_one


# ---------------------------------------------------------------- vs the reference
@pytest.fixture(scope="module")
def fixtures():
    z = gold("updates_hoprec")
    return {tag: Trials(z, tag) for tag in TAGS}


@pytest.mark.parametrize("tag", TAGS)
def test_single_sample_vs_reference_1e5(smore, fixtures, tag):
    F = fixtures[tag]
    g, field, pn = make_pair(smore, "pl3" if tag == "pl3" else "bip")
    pn.alloc_tables(F.dim, 1)
    left_out = 0
    for t in range(F.n):
        s, _slots, _kind, _rej, _rec, pbits, T0, want = F.trial(t)
        if F.run(T0.copy(), s).margin < 1e-4:   # fp64 margin of some gate
            left_out += 1
            continue
        pn.set_table(0, T0.astype(np.float32))
        t0, p0 = pn.hoprec_stats()
        pn.train_hoprec(s, 1, TOTAL, F.steps, F.alpha, F.seed, "serial")
        np.testing.assert_allclose(pn.get_table(0), want, atol=1e-5, rtol=0, err_msg="%s trial %d" % (tag, t))
        assert pn.hoprec_stats() == (t0 + 5 * F.steps, p0 + int(pbits.sum()))
    assert left_out <= 0.05 * F.n


def test_closed_gates_change_nothing(smore, fixtures):
    F = fixtures["bip16"]
    g, field, pn = make_pair(smore, "bip")
    pn.alloc_tables(F.dim, 1)
    seen = 0
    for t in range(F.n):
        s, _slots, kind, *_rest, T0, _want = F.trial(t)
        if not kind:
            continue
        seen += 1
        T0 = T0.astype(np.float32)
        for mode in ("serial", "atomic"):
            pn.set_table(0, T0)
            t0, p0 = pn.hoprec_stats()
            pn.train_hoprec(s, 1, TOTAL, F.steps, F.alpha, F.seed, mode)
            assert pn.get_table(0).tobytes() == T0.tobytes()
            assert pn.hoprec_stats() == (t0 + 5 * F.steps, p0)
    assert seen >= 3


# ---------------------------------------------------------------- scatter quality
# The bar is the CPU fp32 spec's AUC (hoprec_spec.SPEC_AUC: 0.9115, 0.9065,
# 0.9105 at seeds SEED .. SEED + 2, recomputed by test_hoprec_cpu.py), not a
# GPU run: spread 0.005, so a GPU run must reach 0.9065 - 3 x 0.005 = 0.8915.
# hs.SPEC_AUC is a recorded constant: this file alone would not notice it going stale --
# tests/test_hoprec_cpu.py::test_recorded_spec_auc_is_what_the_fp32_spec_gives recomputes
# the three values from the spec to 5e-5 in the CPU suite.
# (The MI355X at seed SEED: atomic 0.9120, hybrid 0.9115.)
AUC_BAR = min(hs.SPEC_AUC) - 3 * (max(hs.SPEC_AUC) - min(hs.SPEC_AUC))


@pytest.mark.parametrize("mode", ["atomic", "hybrid"])
def test_atomic_scatter_reaches_spec_quality(smore, mode):
    g, field, pn = make_pair(smore, "bip")
    pn.alloc_tables(hs.AUC_DIM, 1)
    pn.init_table_glibc(0, 0)
    np.testing.assert_array_equal(pn.get_table(0), hs.glibc_table(g.V, hs.AUC_DIM))   # the spec runs' start
    pn.train_hoprec(0, hs.AUC_SAMPLES, hs.AUC_SAMPLES, hs.AUC_STEPS, 0.025, SEED, mode)
    T = pn.get_table(0)
    assert np.isfinite(T).all()
    assert pn.last_mode() == "atomic"   # hybrid: the atomic scatter, and it says so
    tested, passed = pn.hoprec_stats()
    assert tested == 5 * hs.AUC_STEPS * hs.AUC_SAMPLES and 0 < passed < tested
    a = hs.auc(g, field, T)
    print("AUC %s %.4f; fp32 spec %s, bar %.4f; gates passed per sample %.2f"
          % (mode, a, hs.SPEC_AUC, AUC_BAR, passed / hs.AUC_SAMPLES))
    assert abs(AUC_BAR - 0.8915) < 1e-9
    assert a >= AUC_BAR, (mode, a, hs.SPEC_AUC)


# ---------------------------------------------------------------- refusals
def test_refusals(smore):
    from smore_amd import _lib
    SmoreError = _lib.SmoreError
    pn = smore.ProNet(0)
    with pytest.raises(SmoreError, match="no graph"):
        pn.train_hoprec(0, 10, 100, 5, 0.025, SEED, "serial")
    pn.SetNegativeMethod("no_degrees")
    pn.LoadEdgeList(os.path.join(GOLDEN, "bip.txt"), 1)
    with pytest.raises(SmoreError, match="tables not allocated"):
        pn.train_hoprec(0, 10, 100, 5, 0.025, SEED, "serial")
    pn.alloc_tables(8, 1)
    with pytest.raises(SmoreError, match="no fields"):
        pn.train_hoprec(0, 10, 100, 5, 0.025, SEED, "serial")
    with pytest.raises(SmoreError, match="no fields"):
        pn.hoprec_records(0, 10, 5, SEED)
    # fields under which no sample could start: every vertex with source mass outside field 0
    f = np.ones(pn.MAX_vid, np.int32)
    pn.set_fields(f, 2)
    rc = _lib.lib.smore_train_hoprec(pn.ctx, 0, 10, 100, 5, 0.025, SEED, _lib.MODE["serial"])
    assert rc == _lib.ESTATE and b"source mass" in _lib.lib.smore_last_error(pn.ctx)
    pn.LoadFieldMeta(os.path.join(GOLDEN, "bip_field.txt"))
    with pytest.raises(SmoreError, match="total == 0"):
        pn.train_hoprec(0, 10, 0, 5, 0.025, SEED, "serial")
    for bad in (-1, 4):
        rc = _lib.lib.smore_train_hoprec(pn.ctx, 0, 10, 100, 5, 0.025, SEED, bad)
        assert rc == _lib.EINVAL and b"bad mode" in _lib.lib.smore_last_error(pn.ctx)
    for steps in (0, 11):
        rc = _lib.lib.smore_train_hoprec(pn.ctx, 0, 10, 100, steps, 0.025, SEED, _lib.MODE["serial"])
        assert rc == _lib.EINVAL and b"walk_steps" in _lib.lib.smore_last_error(pn.ctx)
        with pytest.raises(SmoreError, match="walk_steps"):
            pn.hoprec_records(0, 10, steps, SEED)
    rc = _lib.lib.smore_train_hoprec(pn.ctx, 0, 10, 100, 5, 0.025, SEED, _lib.MODE["hogwild"])
    assert rc == _lib.EINVAL and b"plain-store" in _lib.lib.smore_last_error(pn.ctx)
    pn.set_semantics("go")
    with pytest.raises(SmoreError, match="Go semantics"):
        pn.train_hoprec(0, 10, 100, 5, 0.025, SEED, "serial")
    pn.set_semantics("cpp")
    pn.census_begin()
    with pytest.raises(SmoreError, match="census"):
        pn.train_hoprec(0, 10, 100, 5, 0.025, SEED, "serial")
    pn.census_end(1.0)
    pn.train_hoprec(0, 10, 100, 5, 0.025, SEED, "serial")   # and now it runs
    assert pn.hoprec_stats()[0] == 10 * 25


# ---------------------------------------------------------------- model class and CLI
CLS_SAMPLES, CLS_DIM, CLS_STEPS = 20000, 8, 5


@pytest.fixture(scope="module")
def run_spec32():
    z = gold("e2e_hoprec_bip")   # its W0 is the reference's own Init of bip.txt at d = 8
    g = hs.graph("bip.txt")
    T = hs.padded(z["W0"].astype(np.float32), CLS_DIM)
    r = hs.run(g, z["field"], T, CLS_STEPS, 0.025, CLS_SAMPLES, 0, CLS_SAMPLES, SEED)
    raw, off = bytes(z["names"]), z["name_off"]
    names = [raw[off[k]:off[k + 1]].decode() for k in range(len(off) - 1)]
    return z, T[:, :CLS_DIM], names, (r.tested, r.npassed)


def test_model_class_vs_fp32_spec(smore, run_spec32, capsys):
    z, want, names, stats = run_spec32
    m = smore.HBPR(0, "serial", SEED)
    assert m.pnet.negative_method == "no_degrees"
    m.LoadEdgeList(os.path.join(GOLDEN, "bip.txt"), 1)
    m.LoadFieldMeta(os.path.join(GOLDEN, "bip_field.txt"))
    m.Init(CLS_DIM)
    np.testing.assert_array_equal(m.w_vertex, z["W0"].astype(np.float32))   # the reference's own Init
    m.Train(1, CLS_STEPS, 0.025, 1, samples=CLS_SAMPLES)
    out = capsys.readouterr().out
    assert "[HBPR]" in out and "walk steps:" in out and "Progress: 100.000 %" in out
    np.testing.assert_array_equal(m.w_vertex, want)
    assert m.pnet.hoprec_stats() == stats
    assert [m.pnet.vertex_name(v) for v in range(len(names))] == names


def test_cli_vs_fp32_spec(run_spec32, tmp_path):
    _z, want, names, _stats = run_spec32
    out = str(tmp_path / "rep.txt")
    r = subprocess.run([os.path.join(BIN, "hoprec"), "-train", os.path.join(GOLDEN, "bip.txt"), "-field",
                        os.path.join(GOLDEN, "bip_field.txt"), "-save", out, "-dimensions", str(CLS_DIM),
                        "-sample_times", "1", "-walk_steps", str(CLS_STEPS), "-alpha", "0.025", "-threads", "1",
                        "-seed", str(SEED), "-mode", "serial", "-samples", str(CLS_SAMPLES)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for heading in ("Connections:", "Meta Data Preview:", "# of meta data:\t\t295", "Meta Data Loading:", "# of field:\t\t2", "Model Setting:", "[HBPR]",
                    "Learning Parameters:", "walk steps:\t\t5", "Start Training:", "Save Model:", "Save to <"):
        assert heading in r.stdout, heading
    lines = open(out).read().splitlines()
    assert lines[0].split() == [str(len(names)), str(CLS_DIM)]
    assert [ln.split()[0] for ln in lines[1:]] == names
    W = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[1:]])
    # the saved text is %g: 6 significant digits, relative 5e-6
    assert (np.abs(W - want) <= 5e-6 * np.abs(want) + 1e-30).all(), np.abs(W - want).max()


def test_cli_usage_and_gpus():
    r = subprocess.run([os.path.join(BIN, "hoprec")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage:" in r.stdout and "-field" in r.stdout and "-walk_steps" in r.stdout
    r = subprocess.run([os.path.join(BIN, "hoprec"), "-train", os.path.join(GOLDEN, "bip.txt"), "-field",
                        os.path.join(GOLDEN, "bip_field.txt"), "-save", "/dev/null", "-gpus", "2"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "one GPU" in r.stderr
