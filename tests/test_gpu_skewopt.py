"""Skew-OPT on the GPU (smore_train_skewopt, smore_amd.SPR, bin/skewopt) against
the rule's CPU spec (tests/c/skewopt_spec.c) and the reference's own runs
(tests/golden/updates_skewopt.npz, e2e_skewopt_bip.npz).  Needs an MI355X.

  * serial mode vs the fp32 spec               : bit-exact, counters included
  * one update vs the reference (fp64)         : 1e-5 absolute, same decisions
  * all-gated samples                          : table bytes unchanged
  * g == 0                                     : finite, the fp32 spec's bits
  * atomic / hybrid scatter                    : ranking AUC of the serial run
  * 10^6-sample run vs the reference           : NOT compared -- the fp32 and
    fp64 runs part ways at a gate decision after 43389 samples
    (test_skewopt_cpu.py); the model class and the CLI are
    held to the fp32 spec of the same run instead
"""
import os
import subprocess

import numpy as np
import pytest

from tests import skewopt_spec as ss
from tests.conftest import GOLDEN, ROOT
from tests.test_gpu_warp import auc

pytestmark = pytest.mark.gpu

SEED = 20251015
BIN = os.path.join(ROOT, "smore_amd", "bin")
TOTAL1 = ss.TOTAL   # single-sample trials: alpha stays alpha0


@pytest.fixture(scope="module")
def smore():
    import smore_amd
    return smore_amd


def make_pair(smore, fname):
    g = ss.graph(fname)
    pn = smore.ProNet(0)
    pn.SetNegativeMethod("no_degrees")
    pn.LoadEdgeList(os.path.join(GOLDEN, fname), 0)
    assert pn.MAX_vid == g.V
    return g, pn


def spread(dim):
    """(xi, omega, eta) that spread g over gate, clamp and interior on the LCG
    table: f has standard deviation sqrt(dim / 72), omega is about 0.4 of it."""
    return 0.05, 0.05 * dim ** 0.5, 3


# ---------------------------------------------------------------- vs the fp32 spec
# d = 5: G = 2 with a padded element; 64 / 128: four / two groups per wave; 300:
# G = 64, two registers per lane, the second chunk round partly past dpad, and
# the negative rows in two batches of eight
@pytest.mark.parametrize("fname,dim", [("toy.txt", 5), ("bip.txt", 5), ("bip.txt", 64), ("bip.txt", 128),
                                       ("bip.txt", 300)])
def test_serial_bit_exact_vs_fp32_spec(smore, fname, dim):
    g, pn = make_pair(smore, fname)
    xi, omega, eta = spread(dim)
    W0 = ss.lcg_table(g.V, dim).astype(np.float32)
    pn.alloc_tables(dim, 1)
    pn.set_table(0, W0)
    total, begin, n = 10 ** 6, 9000, 3000   # crosses the first alpha step at 10^4
    sk0 = pn.skipped()
    pn.train_skewopt(begin, n, total, 0.005, xi, omega, eta, SEED, "serial")
    W = ss.padded(W0, dim)
    r = ss.run(g, W, 0.005, xi, omega, eta, total, begin, begin + n, SEED)
    assert np.isfinite(W).all()
    # the run met gated, clamped and interior negatives (clamps are rare at d = 5)
    kinds = [int((r.kind == k).sum()) for k in (0, 1, 2)]
    assert kinds[0] > n // 20 and kinds[1] > 0 and kinds[2] > n // 20, kinds
    if fname == "bip.txt":   # both paths of the kernel ran
        d = ss.distinct(r.rec)
        assert d.sum() > n // 10 and (~d).sum() > n // 10, (d.sum(), n)
    np.testing.assert_array_equal(pn.get_table(0), W[:, :dim])
    assert pn.skewopt_stats() == (r.passed, r.updated)
    assert pn.skipped() - sk0 == r.skipped
    assert pn.last_mode() == "serial"


def test_chunk_independence(smore):
    g, pn = make_pair(smore, "bip.txt")
    xi, omega, eta = spread(64)
    W0 = ss.lcg_table(g.V, 64).astype(np.float32)
    pn.alloc_tables(64, 1)
    pn.set_table(0, W0)
    pn.train_skewopt(0, 2000, 10 ** 6, 0.005, xi, omega, eta, SEED, "serial")
    one, st_one = pn.get_table(0), pn.skewopt_stats()
    pn.alloc_tables(64, 1)   # zeroes the counters
    assert pn.skewopt_stats() == (0, 0)
    pn.set_table(0, W0)
    pn.train_skewopt(0, 777, 10 ** 6, 0.005, xi, omega, eta, SEED, "serial")
    pn.train_skewopt(777, 2000 - 777, 10 ** 6, 0.005, xi, omega, eta, SEED, "serial")
    np.testing.assert_array_equal(pn.get_table(0), one)
    assert pn.skewopt_stats() == st_one and st_one[1] > 0


# ---------------------------------------------------------------- vs the reference
def test_single_update_vs_reference_1e5(smore):
    z = ss.gold("updates_skewopt")
    out = ss.left_out()
    total = 0
    for tag in ss.tags(z):
        tr = ss.Trials(z, tag)
        _g, pn = make_pair(smore, tr.gfile)
        pn.alloc_tables(tr.dim, 1)
        for t in range(tr.n):
            total += 1
            if (tag, t) in out:
                continue
            s, _gated, _up, _ids, _p, T0, want = tr.trial(t)
            pn.set_table(0, T0.astype(np.float32))
            pn.train_skewopt(s, 1, TOTAL1, tr.alpha, tr.xi, tr.omega, tr.eta, tr.seed, "serial")
            np.testing.assert_allclose(pn.get_table(0), want, atol=1e-5, rtol=0, err_msg="%s trial %d" % (tag, t))
    assert len(out) <= 0.05 * total


def test_all_gated_changes_nothing(smore):
    z = ss.gold("updates_skewopt")
    seen = 0
    for tag in ss.tags(z):
        tr = ss.Trials(z, tag)
        pn = None
        for t in range(tr.n):
            s, gated, _up, _ids, _p, T0, _want = tr.trial(t)
            if not gated:
                continue
            if pn is None:
                _g, pn = make_pair(smore, tr.gfile)
                pn.alloc_tables(tr.dim, 1)
            seen += 1
            T0 = T0.astype(np.float32)
            pn.set_table(0, T0)
            st0 = pn.skewopt_stats()
            pn.train_skewopt(s, 1, TOTAL1, tr.alpha, tr.xi, tr.omega, tr.eta, tr.seed, "serial")
            assert pn.get_table(0).tobytes() == T0.tobytes()
            assert pn.skewopt_stats() == st0
    assert seen >= 3


@pytest.mark.parametrize("eta", [1, 2, 3])
def test_g_zero_equals_fp32_spec(smore, eta):
    g, dim, s, ids, xi, omega, alpha, seed = ss.gzero_case()
    _g, pn = make_pair(smore, "bip.txt")
    T0 = ss.gzero_table(g.V, dim, int(ids[0]), int(ids[1]), xi).astype(np.float32)
    pn.alloc_tables(dim, 1)
    pn.set_table(0, T0)
    pn.train_skewopt(s, 1, TOTAL1, alpha, xi, omega, eta, seed, "serial")
    W = ss.padded(T0, dim)
    r = ss.run(g, W, alpha, xi, omega, eta, TOTAL1, s, s + 1, seed)
    assert r.gmin == 0.0
    T = pn.get_table(0)
    assert np.isfinite(T).all() and T.tobytes() == W[:, :dim].tobytes()
    assert pn.skewopt_stats() == (r.passed, r.updated)


# ---------------------------------------------------------------- scatter modes
# SPR::Init's table, 200 000 samples at the defaults, d = 32, seeds SEED, SEED + 1, SEED + 2,
# test_gpu_warp.py's AUC (every training positive against one uniform negative).
# Serial: 0.80775, 0.81075, 0.81075 (the fp32 spec's values, which the serial kernel
# reproduces bit for bit): spread 0.003, margin = 3 x spread.  The atomic values measured on
# the MI355X are in DESIGN.md 12c.
AUC_MARGIN = 0.009


def auc_run(smore, mode, seed):
    g, pn = make_pair(smore, "bip.txt")
    pn.alloc_tables(ss.AUC_DIM, 1)
    pn.init_table_glibc_offset(0, 0, 0.01)
    pn.train_skewopt(0, ss.AUC_SAMPLES, ss.AUC_SAMPLES, 0.025, 10.0, 3.0, 3, seed, mode)
    return g, pn, pn.get_table(0)


@pytest.fixture(scope="module")
def serial_auc(smore):
    g, _pn, T = auc_run(smore, "serial", SEED)
    return auc(g, T)


@pytest.mark.parametrize("mode", ["atomic", "hybrid"])
def test_parallel_modes_reach_serial_quality(smore, serial_auc, mode):
    g, pn, T = auc_run(smore, mode, SEED)
    assert np.isfinite(T).all()
    assert pn.last_mode() == "atomic"   # hybrid: the atomic scatter, and it says so
    passed, updated = pn.skewopt_stats()
    assert 0 < updated <= ss.AUC_SAMPLES and updated <= passed <= 16 * ss.AUC_SAMPLES
    a = auc(g, T)
    print("AUC %s %.4f serial %.4f" % (mode, a, serial_auc))
    assert serial_auc > 0.6   # the run learnt something to compare
    assert a >= serial_auc - AUC_MARGIN, (mode, a, serial_auc)


# ---------------------------------------------------------------- refusals
def test_refusals(smore):
    from smore_amd import _lib
    SmoreError = _lib.SmoreError
    pn = smore.ProNet(0)
    with pytest.raises(SmoreError, match="no graph"):
        pn.train_skewopt(0, 10, 100, 0.025, 10.0, 3.0, 3, SEED, "serial")
    pn.SetNegativeMethod("no_degrees")
    pn.LoadEdgeList(os.path.join(GOLDEN, "bip.txt"), 0)
    with pytest.raises(SmoreError, match="tables not allocated"):
        pn.train_skewopt(0, 10, 100, 0.025, 10.0, 3.0, 3, SEED, "serial")
    pn.alloc_tables(8, 1)
    with pytest.raises(SmoreError, match="total == 0"):
        pn.train_skewopt(0, 10, 0, 0.025, 10.0, 3.0, 3, SEED, "serial")
    call = _lib.lib.smore_train_skewopt
    for bad in (-1, 4):
        rc = call(pn.ctx, 0, 10, 100, 0.025, 10.0, 3.0, 3, SEED, bad)
        assert rc == _lib.EINVAL and b"bad mode" in _lib.lib.smore_last_error(pn.ctx)
        with pytest.raises(SmoreError):
            _lib.check(pn.ctx, rc, "train_skewopt")
    rc = call(pn.ctx, 0, 10, 100, 0.025, 10.0, 0.0, 3, SEED, _lib.MODE["serial"])
    assert rc == _lib.EINVAL and b"omega == 0" in _lib.lib.smore_last_error(pn.ctx)
    with pytest.raises(SmoreError, match="omega == 0"):
        pn.train_skewopt(0, 10, 100, 0.025, 10.0, 0.0, 3, SEED, "serial")
    for eta in (0, -2):
        rc = call(pn.ctx, 0, 10, 100, 0.025, 10.0, 3.0, eta, SEED, _lib.MODE["serial"])
        assert rc == _lib.EINVAL and b"eta < 1" in _lib.lib.smore_last_error(pn.ctx)
    with pytest.raises(SmoreError, match="eta < 1"):
        pn.train_skewopt(0, 10, 100, 0.025, 10.0, 3.0, 0, SEED, "serial")
    rc = call(pn.ctx, 0, 10, 100, 0.025, 10.0, 3.0, 3, SEED, _lib.MODE["hogwild"])
    assert rc == _lib.EINVAL and b"no plain-store scatter" in _lib.lib.smore_last_error(pn.ctx)
    with pytest.raises(SmoreError, match="no plain-store scatter"):
        pn.train_skewopt(0, 10, 100, 0.025, 10.0, 3.0, 3, SEED, "hogwild")
    pn.set_semantics("go")
    with pytest.raises(SmoreError, match="Go semantics"):
        pn.train_skewopt(0, 10, 100, 0.025, 10.0, 3.0, 3, SEED, "serial")
    pn.set_semantics("cpp")
    pn.census_begin()
    with pytest.raises(SmoreError, match="census"):
        pn.train_skewopt(0, 10, 100, 0.025, 10.0, 3.0, 3, SEED, "serial")
    pn.census_end(1.0)
    pn.init_table_glibc_offset(0, 0, 0.01)
    pn.train_skewopt(0, 10, 100, 0.025, 10.0, 3.0, 3, SEED, "serial")   # and now it runs
    assert 0 < pn.skewopt_stats()[1] <= 10


# ---------------------------------------------------------------- model class and CLI
@pytest.fixture(scope="module")
def e2e_spec32():
    z = ss.gold("e2e_skewopt_bip")
    dim, st, eta, seed = (int(x) for x in z["meta"])
    alpha, xi, omega = (float(x) for x in z["meta_f"])
    g = ss.graph("bip.txt")
    T = ss.padded(z["W0"].astype(np.float32), dim)
    r = ss.run(g, T, alpha, xi, omega, eta, st * 10 ** 6, 0, st * 10 ** 6, seed)
    raw, off = bytes(z["names"]), z["name_off"]
    names = [raw[off[k]:off[k + 1]].decode() for k in range(len(off) - 1)]
    return z, dim, st, seed, (alpha, xi, omega, eta), T[:, :dim], names, (r.passed, r.updated)


def test_model_class_vs_fp32_spec(smore, e2e_spec32, capsys):
    z, dim, st, seed, (alpha, xi, omega, eta), want, names, stats = e2e_spec32
    m = smore.SPR(0, "serial", seed)
    assert m.pnet.negative_method == "no_degrees"
    m.LoadEdgeList(os.path.join(GOLDEN, "bip.txt"), 0)
    m.Init(dim)
    np.testing.assert_array_equal(m.w_vertex, z["W0"].astype(np.float32))   # the reference's own Init
    m.Train(st, 5, alpha, 0.01, xi, omega, eta, 1)
    out = capsys.readouterr().out
    assert "[Skew-OPT]" in out and "regularization:" in out and "Progress: 100.000 %" in out
    assert "xi:" in out and "omega:" in out and "eta:" in out
    np.testing.assert_array_equal(m.w_vertex, want)
    assert m.pnet.skewopt_stats() == stats
    assert [m.pnet.vertex_name(v) for v in range(len(names))] == names


def test_cli_vs_fp32_spec(e2e_spec32, tmp_path):
    z, dim, st, seed, (alpha, xi, omega, eta), want, names, _stats = e2e_spec32
    out = str(tmp_path / "rep.txt")
    r = subprocess.run([os.path.join(BIN, "skewopt"), "-train", os.path.join(GOLDEN, "bip.txt"), "-save", out,
                        "-dimensions", str(dim), "-sample_times", str(st), "-alpha", repr(alpha), "-reg", "0.01",
                        "-xi", repr(xi), "-omega", repr(omega), "-eta", str(eta), "-threads", "1",
                        "-seed", str(seed), "-mode", "serial"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[Skew-OPT]" in r.stdout and "Save to <" in r.stdout
    lines = open(out).read().splitlines()
    assert lines[0].split() == [str(len(names)), str(dim)]
    assert [ln.split()[0] for ln in lines[1:]] == names
    W = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[1:]])
    # the saved text is %g: 6 significant digits, relative 5e-6
    assert (np.abs(W - want) <= 5e-6 * np.abs(want) + 1e-30).all(), np.abs(W - want).max()


def test_cli_usage_and_gpus():
    r = subprocess.run([os.path.join(BIN, "skewopt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage:" in r.stdout
    r = subprocess.run([os.path.join(BIN, "skewopt"), "-train", os.path.join(GOLDEN, "bip.txt"), "-save", "/dev/null",
                        "-gpus", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "one GPU" in r.stderr
