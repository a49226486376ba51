"""WARP on the GPU (smore_train_warp, smore_amd.WARP, bin/warp) against the
rule's CPU spec (tests/c/warp_spec.c) and the reference's own runs
(tests/golden/updates_warp.npz, e2e_warp_bip.npz).  Needs an MI355X.

  * serial mode vs the fp32 spec               : bit-exact, counters included
  * one update vs the reference (fp64)         : 1e-5 absolute, margin >= 1e-4
  * exhaustion (32 trials, all f >= 1)         : table bytes unchanged
  * atomic / hogwild scatter                   : ranking AUC of the serial run
  * 10^6-sample run vs the reference           : NOT compared -- the fp32 and
    fp64 runs part ways at a margin decision after 65769 samples
    (test_warp_cpu.py, DESIGN.md "WARP"); the model class and the CLI are
    held to the fp32 spec of the same run instead
"""
import os
import subprocess

import numpy as np
import pytest

from tests import warp_spec as ws
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SEED = 20251015
BIN = os.path.join(ROOT, "smore_amd", "bin")
TOTAL1 = 10 ** 9   # single-sample trials: alpha stays alpha0


def gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def smore():
    import smore_amd
    return smore_amd


def make_pair(smore, fname):
    g = ws.graph(fname)
    pn = smore.ProNet(0)
    pn.SetNegativeMethod("no_degrees")
    pn.LoadEdgeList(os.path.join(GOLDEN, fname), 0)
    assert pn.MAX_vid == g.V
    return g, pn


# ---------------------------------------------------------------- vs the fp32 spec
# d = 5: G = 2 with a padded element; 64 / 128: four / two groups per wave that
# leave the trial loop apart; 300: G = 64, two registers per lane, the second
# chunk round partly past dpad
@pytest.mark.parametrize("fname,dim", [("toy.txt", 5), ("bip.txt", 5), ("bip.txt", 64), ("bip.txt", 128),
                                       ("bip.txt", 300)])
def test_serial_bit_exact_vs_fp32_spec(smore, fname, dim):
    g, pn = make_pair(smore, fname)
    W0 = ws.lcg_table(g.V, dim).astype(np.float32)
    pn.alloc_tables(dim, 1)
    pn.set_table(0, W0)
    total, begin, n = 10 ** 6, 9000, 3000   # crosses the first alpha step at 10^4
    sk0 = pn.skipped()
    pn.train_warp(begin, n, total, 0.05, SEED, "serial")
    W = ws.padded(W0, dim)
    nt, _m, trials, updated, skipped = ws.run(g, W, 0.05, total, begin, begin + n, SEED)
    assert (nt > 1).sum() > (0 if dim == 5 else n // 20)   # multi-trial loops really ran
    np.testing.assert_array_equal(pn.get_table(0), W[:, :dim])
    assert pn.warp_stats() == (trials, updated)
    assert pn.skipped() - sk0 == skipped
    assert pn.last_mode() == "serial"


def test_chunk_independence(smore):
    g, pn = make_pair(smore, "bip.txt")
    W0 = ws.lcg_table(g.V, 64).astype(np.float32)
    pn.alloc_tables(64, 1)
    pn.set_table(0, W0)
    pn.train_warp(0, 2000, 10 ** 6, 0.05, SEED, "serial")
    one, st_one = pn.get_table(0), pn.warp_stats()
    pn.alloc_tables(64, 1)   # zeroes the counters
    assert pn.warp_stats() == (0, 0)
    pn.set_table(0, W0)
    pn.train_warp(0, 777, 10 ** 6, 0.05, SEED, "serial")
    pn.train_warp(777, 2000 - 777, 10 ** 6, 0.05, SEED, "serial")
    np.testing.assert_array_equal(pn.get_table(0), one)
    assert pn.warp_stats() == st_one


# ---------------------------------------------------------------- vs the reference
def _trials(z, tag):
    dim, seed, _first, n, nx = (int(x) for x in z["meta_" + tag])
    return tag + ".txt", dim, seed, float(z["meta_" + tag + "_f"][0]), n + nx


def _start(z, tag, t):
    _s, v, i, _j0, _slots, ex = (int(x) for x in z[tag + "_trial"][t])
    W0 = z[tag + "_W0"]
    return ws.exhaustion_table(W0.shape[0], W0.shape[1], v, i) if ex else W0.copy()


@pytest.mark.parametrize("tag", ["bip", "toy"])
def test_single_update_vs_reference_1e5(smore, tag):
    z = gold("updates_warp")
    fname, dim, seed, alpha, n = _trials(z, tag)
    g, pn = make_pair(smore, fname)
    pn.alloc_tables(dim, 1)
    skipped = 0
    for t in range(n):
        s, v, i, _j0, _slots, ex = (int(x) for x in z[tag + "_trial"][t])
        T0 = _start(z, tag, t)
        want = T0.copy()
        if ws.run(g, T0.copy(), alpha, TOTAL1, s, s + 1, seed)[1] < 1e-4:   # fp64 margin
            skipped += 1
            continue
        if not ex:   # an exhaustion trial changes nothing
            want[v], want[i], want[int(z[tag + "_jlast"][t])] = z[tag + "_rows"][t]
        pn.set_table(0, T0.astype(np.float32))
        pn.train_warp(s, 1, TOTAL1, alpha, seed, "serial")
        np.testing.assert_allclose(pn.get_table(0), want, atol=1e-5, rtol=0, err_msg="%s trial %d" % (tag, t))
    assert skipped <= 0.05 * n


def test_exhaustion_changes_nothing(smore):
    z = gold("updates_warp")
    fname, dim, seed, alpha, n = _trials(z, "bip")
    g, pn = make_pair(smore, fname)
    pn.alloc_tables(dim, 1)
    seen = 0
    for t in range(n):
        s, v, i, _j0, _slots, ex = (int(x) for x in z["bip_trial"][t])
        if not ex:
            continue
        seen += 1
        T0 = _start(z, "bip", t).astype(np.float32)
        pn.set_table(0, T0)
        tr0, up0 = pn.warp_stats()
        pn.train_warp(s, 1, TOTAL1, alpha, seed, "serial")
        assert pn.get_table(0).tobytes() == T0.tobytes()
        assert pn.warp_stats() == (tr0 + 32, up0)
    assert seen >= 3


# ---------------------------------------------------------------- scatter modes
AUC_SAMPLES, AUC_DIM = 200000, 32
# the atomic run at seeds SEED, SEED + 1, SEED + 2 reached AUC 0.81225, 0.80925, 0.80325 on
# the MI355X (serial: 0.81225, 0.80725, 0.80425): spread 0.009, margin = 3 x spread
AUC_MARGIN = 0.027


def auc(g, T, seed=5):
    """Every training positive (u -> i) against one uniform negative."""
    u = np.repeat(np.arange(g.V), np.diff(g.offsets))
    i = g.targets[:g.E]
    j = np.random.default_rng(seed).integers(0, g.V, len(u))
    T = T.astype(np.float64)
    x = (T[u] * (T[i] - T[j])).sum(1)
    return float((x > 0).mean() + 0.5 * (x == 0).mean())


def auc_run(smore, mode, seed):
    g, pn = make_pair(smore, "bip.txt")
    pn.alloc_tables(AUC_DIM, 1)
    pn.init_table_glibc(0, 0)
    pn.train_warp(0, AUC_SAMPLES, AUC_SAMPLES, 0.025, seed, mode)
    T = pn.get_table(0)
    return g, pn, T


@pytest.fixture(scope="module")
def serial_auc(smore):
    g, _pn, T = auc_run(smore, "serial", SEED)
    return auc(g, T)


@pytest.mark.parametrize("mode,ran", [("atomic", "atomic"), ("hogwild", "hogwild"), ("hybrid", "atomic")])
def test_hogwild_modes_reach_serial_quality(smore, serial_auc, mode, ran):
    """Every scatter reaches the serial run's AUC.  Plain stores do so only
    under the driver's cap on groups in flight (effective rows / 32, one group
    on this 295-vertex graph): uncapped, one block's 32 groups reached 0.481 /
    0.488 / 0.478 at three seeds against the serial run's 0.812 / 0.807 /
    0.804, two groups 0.775 (DESIGN.md 12a "Scatter quality")."""
    g, pn, T = auc_run(smore, mode, SEED)
    assert np.isfinite(T).all()
    assert pn.last_mode() == ran   # hybrid: the atomic scatter, and it says so
    trials, updated = pn.warp_stats()
    assert 0 < updated <= AUC_SAMPLES and updated <= trials <= 32 * AUC_SAMPLES
    a = auc(g, T)
    print("AUC %s %.4f serial %.4f" % (mode, a, serial_auc))
    assert serial_auc > 0.6   # the run learnt something to compare
    assert a >= serial_auc - AUC_MARGIN, (mode, a, serial_auc)


def test_phase_times_after_warp(smore):
    import ctypes as C
    from smore_amd import _lib
    _g, pn = make_pair(smore, "bip.txt")
    pn.alloc_tables(16, 1)
    pn.init_table_glibc(0, 0)
    pn.train_warp(0, 50000, 50000, 0.025, SEED, "hogwild")
    d, u, n = C.c_float(), C.c_float(), C.c_int()
    assert _lib.lib.smore_last_phase_ms(pn.ctx, C.byref(d), C.byref(u), C.byref(n)) == _lib.OK
    assert n.value == 1 and d.value >= 0 and u.value > 0


# ---------------------------------------------------------------- refusals
def test_refusals(smore):
    from smore_amd import _lib
    SmoreError = _lib.SmoreError
    pn = smore.ProNet(0)
    with pytest.raises(SmoreError, match="no graph"):
        pn.train_warp(0, 10, 100, 0.025, SEED, "serial")
    pn.SetNegativeMethod("no_degrees")
    pn.LoadEdgeList(os.path.join(GOLDEN, "bip.txt"), 0)
    with pytest.raises(SmoreError, match="tables not allocated"):
        pn.train_warp(0, 10, 100, 0.025, SEED, "serial")
    pn.alloc_tables(8, 1)
    with pytest.raises(SmoreError, match="total == 0"):
        pn.train_warp(0, 10, 0, 0.025, SEED, "serial")
    for bad in (-1, 4):
        rc = _lib.lib.smore_train_warp(pn.ctx, 0, 10, 100, 0.025, SEED, bad)
        assert rc == _lib.EINVAL and b"bad mode" in _lib.lib.smore_last_error(pn.ctx)
        with pytest.raises(SmoreError):
            _lib.check(pn.ctx, rc, "train_warp")
    pn.set_semantics("go")
    with pytest.raises(SmoreError, match="Go semantics"):
        pn.train_warp(0, 10, 100, 0.025, SEED, "serial")
    pn.set_semantics("cpp")
    pn.census_begin()
    with pytest.raises(SmoreError, match="census"):
        pn.train_warp(0, 10, 100, 0.025, SEED, "serial")
    pn.census_end(1.0)
    pn.train_warp(0, 10, 100, 0.025, SEED, "serial")   # and now it runs
    assert pn.warp_stats()[0] >= 10 - pn.skipped()


# ---------------------------------------------------------------- model class and CLI
@pytest.fixture(scope="module")
def e2e_spec32():
    z = gold("e2e_warp_bip")
    dim, st, seed = (int(x) for x in z["meta"])
    g = ws.graph("bip.txt")
    T = ws.padded(z["W0"].astype(np.float32), dim)
    _nt, _m, trials, updated, _sk = ws.run(g, T, float(z["meta_f"][0]), st * 10 ** 6, 0, st * 10 ** 6, seed)
    raw, off = bytes(z["names"]), z["name_off"]
    names = [raw[off[k]:off[k + 1]].decode() for k in range(len(off) - 1)]
    return z, dim, st, seed, T[:, :dim], names, (trials, updated)


def test_model_class_vs_fp32_spec(smore, e2e_spec32, capsys):
    z, dim, st, seed, want, names, stats = e2e_spec32
    m = smore.WARP(0, "serial", seed)
    assert m.pnet.negative_method == "no_degrees"
    m.LoadEdgeList(os.path.join(GOLDEN, "bip.txt"), 0)
    m.Init(dim)
    np.testing.assert_array_equal(m.w_vertex, z["W0"].astype(np.float32))   # the reference's own Init
    m.Train(st, 5, float(z["meta_f"][0]), 0.01, 1)
    out = capsys.readouterr().out
    assert "[WARP]" in out and "regularization:" in out and "Progress: 100.000 %" in out
    np.testing.assert_array_equal(m.w_vertex, want)
    assert m.pnet.warp_stats() == stats
    assert [m.pnet.vertex_name(v) for v in range(len(names))] == names


def test_cli_vs_fp32_spec(e2e_spec32, tmp_path):
    z, dim, st, seed, want, names, _stats = e2e_spec32
    out = str(tmp_path / "rep.txt")
    r = subprocess.run([os.path.join(BIN, "warp"), "-train", os.path.join(GOLDEN, "bip.txt"), "-save", out,
                        "-dimensions", str(dim), "-sample_times", str(st), "-alpha", "0.025", "-threads", "1",
                        "-seed", str(seed), "-mode", "serial"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[WARP]" in r.stdout and "Save to <" in r.stdout
    lines = open(out).read().splitlines()
    assert lines[0].split() == [str(len(names)), str(dim)]
    assert [ln.split()[0] for ln in lines[1:]] == names
    W = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[1:]])
    # the saved text is %g: 6 significant digits, relative 5e-6
    assert (np.abs(W - want) <= 5e-6 * np.abs(want) + 1e-30).all(), np.abs(W - want).max()


def test_cli_usage_and_gpus():
    r = subprocess.run([os.path.join(BIN, "warp")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage:" in r.stdout
    r = subprocess.run([os.path.join(BIN, "warp"), "-train", os.path.join(GOLDEN, "bip.txt"), "-save", "/dev/null",
                        "-gpus", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "one GPU" in r.stderr
