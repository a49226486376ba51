"""CSE on the GPU (smore_train_cse, smore_cse_records, smore_amd.NEMF / NERANK,
bin/nemf / bin/nerank) against the rule's CPU spec (tests/c/cse_spec.c) and the
reference's own runs (tests/golden/updates_cse.npz, e2e_*_bip.npz).  Needs an
MI355X.

  * the draw kernel's records and slot counts  : equal to the spec's
  * serial mode vs the fp32 spec               : bit-exact, counters and skipped included
  * one sample vs the reference (fp64)         : 1e-5 absolute
  * all-closed nerank trials                   : WU, WI move by passes A and B only
  * an atomic launch of one sample             : the serial result, one fp32 add per element
  * atomic / hybrid scatter                    : ranking AUC of the CPU fp32 spec
  * class and CLI on the e2e run's first 10^5 samples: the fp32 spec's saved file
"""
import os
import subprocess

import numpy as np
import pytest

from tests import cse_spec as cs
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SEED = 20251015
NEMF, NERANK, TOTAL = cs.NEMF, cs.NERANK, cs.TOTAL
RANKS = (NEMF, NERANK)
BIN = os.path.join(ROOT, "smore_amd", "bin")
GRAPHS = {"bip": ("bip.txt", "bip_field.txt"), "toy": ("toy.txt", "toy_field.txt"),
          "pl3": ("pl100w.txt", "pl100w_field3.txt")}


@pytest.fixture(scope="module")
def smore():
    import smore_amd
    return smore_amd


def make_pair(smore, key):
    gfile, ffile = GRAPHS[key]
    g = cs.graph(gfile)
    field, _n = cs.load_fields(g, ffile)
    pn = smore.ProNet(0)   # out_degrees sources, degrees negatives: the defaults
    pn.LoadEdgeList(os.path.join(GOLDEN, gfile), 1)
    pn.LoadFieldMeta(os.path.join(GOLDEN, ffile))
    assert pn.MAX_vid == g.V
    np.testing.assert_array_equal(pn.fields[0], field)
    return g, field, pn


def put(pn, T):
    for k in range(4):
        pn.set_table(k, T[k])


def get(pn):
    return [pn.get_table(k) for k in range(4)]


def start32(V, dim, rank):
    """fp32 start tables: the trials' LCG stream, WU and WI scaled so that nerank's f spreads
    around its margin and nemf's squared-loss steps stay contractive (alpha |w|^2 < 1)."""
    scale = (288.0 / dim) ** 0.25 if rank else min(1.0, (24.0 / dim) ** 0.5)
    return [t.astype(np.float32) for t in cs.start_tables(V, dim, scale)]


# ---------------------------------------------------------------- the draws
@pytest.mark.parametrize("key", ["bip", "pl3"])
@pytest.mark.parametrize("steps", [1, 5, 10])
def test_records_equal_the_spec(smore, key, steps):
    g, field, pn = make_pair(smore, key)
    for rank in RANKS:
        for begin in (0, (1 << 32) + 12345):   # the second range: a unit counter above 2^32
            n = 20000
            rec, slots = pn.cse_records(rank, begin, n, steps, SEED)
            r = cs.run(g, field, None, steps, rank, 0.025, TOTAL, begin, begin + n, SEED)
            assert rec.shape == (n, cs.width(steps, rank))
            np.testing.assert_array_equal(rec, r.rec)
            np.testing.assert_array_equal(slots, r.slots)
            assert (field[rec[:, 0]] == 0).all()   # every source is a user
            assert (rec[:, cs.nwords(steps, rank):] == -1).all()
            if rank:   # the direct negatives have c's field
                dn = rec[:, 12 * steps:12 * steps + 16]
                assert (field[dn] == field[rec[:, 1]][:, None]).all()
                assert slots.max() > 4 + 10 * 2 * steps + 4 * (steps - 1) + 16   # rejection loops ran


# ---------------------------------------------------------------- vs the fp32 spec
# d = 5: G = 2 with a padded element; 64 / 128: four / two groups per wave; 300: G = 64, two
# registers per lane, the second chunk round partly past dpad; toy and pl3: few vertices, ids
# coincide within a step (the in-order path) and a direct negative equals c
@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("key,dim,steps", [("toy", 5, 5), ("bip", 5, 5), ("bip", 64, 5), ("bip", 128, 5),
                                           ("bip", 300, 5), ("pl3", 8, 3)])
def test_serial_bit_exact_vs_fp32_spec(smore, key, dim, steps, rank):
    g, field, pn = make_pair(smore, key)
    T0 = start32(g.V, dim, rank)
    pn.alloc_tables(dim, 4)
    put(pn, T0)
    total, begin, n = 10 ** 6, 9000, 3000   # crosses the first alpha step at 10^4
    sk0 = pn.skipped()
    pn.train_cse(rank, begin, n, total, steps, 0.025, SEED, "serial")
    T = [cs.padded(t, dim) for t in T0]
    r = cs.run(g, field, T, steps, rank, 0.025, total, begin, begin + n, SEED)
    assert all(np.isfinite(t).all() for t in T)
    got = get(pn)
    for k in range(4):
        np.testing.assert_array_equal(got[k], T[k][:, :dim], err_msg="table %d" % k)
    assert pn.cse_stats() == (r.tested, r.updated)
    if rank:
        assert n <= r.tested and 0 < r.updated <= n
        if key != "toy":
            assert r.tested > n   # some first negatives were gated
    assert pn.skipped() - sk0 == r.skipped
    assert pn.last_mode() == "serial"


@pytest.mark.parametrize("rank", RANKS)
def test_chunk_independence(smore, rank):
    g, field, pn = make_pair(smore, "bip")
    T0 = start32(g.V, 64, rank)
    pn.alloc_tables(64, 4)
    put(pn, T0)
    pn.train_cse(rank, 0, 2000, 10 ** 6, 5, 0.025, SEED, "serial")
    one, st_one = get(pn), pn.cse_stats()
    pn.alloc_tables(64, 4)   # zeroes the counters
    assert pn.cse_stats() == (0, 0)
    put(pn, T0)
    pn.train_cse(rank, 0, 777, 10 ** 6, 5, 0.025, SEED, "serial")
    pn.train_cse(rank, 777, 2000 - 777, 10 ** 6, 5, 0.025, SEED, "serial")
    two = get(pn)
    for k in range(4):
        np.testing.assert_array_equal(two[k], one[k])
    assert pn.cse_stats() == st_one


# ---------------------------------------------------------------- vs the reference
@pytest.fixture(scope="module")
def fixtures():
    return cs.all_trials()


@pytest.mark.parametrize("rank", RANKS)
def test_single_sample_vs_reference_1e5(smore, fixtures, rank):
    left, total = [], 0
    ctx = {}
    for tag in cs.TAGS:
        F = fixtures[rank, tag]
        key = "toy" if tag.startswith("toy") else "bip" if tag.startswith("bip") else "pl3"
        if key not in ctx:
            ctx[key] = make_pair(smore, key)[2]
        pn = ctx[key]
        pn.alloc_tables(F.dim, 4)
        for t in range(F.n):
            s, _slots, _closed, _nd, pidx, _rec, T0, want = F.trial(t)
            total += 1
            put(pn, [x.astype(np.float32) for x in T0])
            t0, u0 = pn.cse_stats()
            pn.train_cse(rank, s, 1, TOTAL, F.steps, F.alpha, F.seed, "serial")
            t1, u1 = pn.cse_stats()
            if rank and (t1 - t0, u1 - u0) != (16 if pidx < 0 else pidx + 1, int(pidx >= 0)):
                left.append((F.key, t))   # the fp32 gates decided other than the reference's
                continue
            for a, b in zip(get(pn), want):
                np.testing.assert_allclose(a, b, atol=1e-5, rtol=0, err_msg="%s trial %d" % (F.key, t))
    print("left out (fp32 gate decides differently): %s of %d" % (left, total))
    assert len(left) <= 0.05 * total


def test_closed_nerank_trials_move_only_what_the_passes_move(smore, fixtures):
    seen = 0
    for tag in cs.TAGS:
        F = fixtures[NERANK, tag]
        closed = [t for t in range(F.n) if F.trial(t)[2]]
        if not closed:
            continue
        pn = make_pair(smore, "bip")[2]
        pn.alloc_tables(F.dim, 4)
        for t in closed:
            s, _slots, _closed, _nd, _pidx, rec, T0, _want = F.trial(t)
            seen += 1
            T0 = [x.astype(np.float32) for x in T0]
            T = [cs.padded(x, F.dim) for x in T0]
            r = F.run(T, s)
            assert (r.tested, r.updated) == (16, 0)
            put(pn, T0)
            t0, u0 = pn.cse_stats()
            pn.train_cse(NERANK, s, 1, TOTAL, F.steps, F.alpha, F.seed, "serial")
            assert pn.cse_stats() == (t0 + 16, u0)
            got = get(pn)
            for k in range(4):
                assert got[k].tobytes() == np.ascontiguousarray(T[k][:, :F.dim]).tobytes()
            # WU and WI: every row but v's / c's keeps its bytes
            others_u = np.arange(F.g.V) != rec[0]
            others_i = np.arange(F.g.V) != rec[1]
            assert got[cs.WU][others_u].tobytes() == T0[cs.WU][others_u].tobytes()
            assert got[cs.WI][others_i].tobytes() == T0[cs.WI][others_i].tobytes()
    assert seen >= 3


@pytest.mark.parametrize("rank", RANKS)
def test_atomic_single_sample_is_serial_plus_one_add(smore, rank):
    """One sample whose row ids are distinct within each table: every row is added to once,
    so the atomic result is orig + fl(new - orig) with new the serial result, exactly."""
    g, field, pn = make_pair(smore, "bip")
    dim, steps = 16, 2
    r = cs.run(g, field, None, steps, rank, 0.05, TOTAL, 1000, 1400, SEED)
    nw = cs.nwords(steps, rank)
    s = None
    for k in range(len(r.rec)):
        rec = r.rec[k]
        per = {cs.WU: [rec[0]], cs.WI: [rec[1]], cs.CI: [rec[0]], cs.CU: [rec[1]]}
        for w in range(2, nw):
            per[cs.table_of_word(w, steps)].append(rec[w])
        if (rec[:nw] >= 0).all() and all(len(set(map(int, v))) == len(v) for v in per.values()):
            s = 1000 + k
            break
    assert s is not None
    T0 = start32(g.V, dim, rank)
    pn.alloc_tables(dim, 4)
    put(pn, T0)
    pn.train_cse(rank, s, 1, TOTAL, steps, 0.05, SEED, "serial")
    serial = get(pn)
    put(pn, T0)
    pn.train_cse(rank, s, 1, TOTAL, steps, 0.05, SEED, "atomic")
    assert pn.last_mode() == "atomic"
    atomic = get(pn)
    moved = 0
    for k in range(4):
        want = T0[k] + (serial[k] - T0[k])   # fp32: one subtraction, one add
        np.testing.assert_array_equal(atomic[k], want, err_msg="table %d" % k)
        moved += int((serial[k] != T0[k]).any(1).sum())
    assert moved >= 2 + 12 * steps


# ---------------------------------------------------------------- scatter quality
# The bar is the CPU fp32 spec's AUC (cse_spec.SPEC_AUC at seeds SEED .. SEED + 2, recomputed
# by test_cse_cpu.py::test_recorded_spec_auc_is_what_the_fp32_spec_gives), not a GPU run:
# its minimum minus three times its spread.  nemf: 0.8980 - 3 x 0.0055 = 0.8815; nerank:
# 0.8200 - 3 x 0.0050 = 0.8050.
def auc_bar(rank):
    a = cs.SPEC_AUC[rank]
    return min(a) - 3 * (max(a) - min(a))


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("mode", ["atomic", "hybrid"])
def test_atomic_scatter_reaches_spec_quality(smore, mode, rank):
    g, field, pn = make_pair(smore, "bip")
    pn.alloc_tables(cs.AUC_DIM, 4)
    pn.init_tables_glibc_pair(0, 1, 0)
    W0 = cs.glibc_tables(g.V, cs.AUC_DIM)
    for k, t in enumerate(get(pn)):
        np.testing.assert_array_equal(t, W0[k])   # the spec runs' start
    pn.train_cse(rank, 0, cs.AUC_SAMPLES, cs.AUC_SAMPLES, cs.AUC_STEPS, 0.025, SEED, mode)
    T = get(pn)
    assert all(np.isfinite(t).all() for t in T)
    assert pn.last_mode() == "atomic"   # hybrid: the atomic scatter, and it says so
    tested, updated = pn.cse_stats()
    if rank:
        assert tested >= cs.AUC_SAMPLES and 0 < updated <= cs.AUC_SAMPLES
    else:
        assert (tested, updated) == (0, 0)
    a = cs.auc(g, field, T[cs.WU], T[cs.WI])
    print("AUC rank %d %s %.4f; fp32 spec %s, bar %.4f" % (rank, mode, a, cs.SPEC_AUC[rank], auc_bar(rank)))
    assert abs(auc_bar(rank) - (0.8050 if rank else 0.8815)) < 1e-9
    assert a >= auc_bar(rank), (mode, a, cs.SPEC_AUC[rank])


# ---------------------------------------------------------------- refusals
def test_refusals(smore):
    from smore_amd import _lib
    SmoreError = _lib.SmoreError
    pn = smore.ProNet(0)
    with pytest.raises(SmoreError, match="no graph"):
        pn.train_cse(0, 0, 10, 100, 5, 0.025, SEED, "serial")
    pn.LoadEdgeList(os.path.join(GOLDEN, "bip.txt"), 1)
    with pytest.raises(SmoreError, match="ntables"):
        pn.alloc_tables(8, 3)
    with pytest.raises(SmoreError, match="four tables"):
        pn.train_cse(0, 0, 10, 100, 5, 0.025, SEED, "serial")
    pn.alloc_tables(8, 2)
    pn.LoadFieldMeta(os.path.join(GOLDEN, "bip_field.txt"))
    rc = _lib.lib.smore_train_cse(pn.ctx, 0, 0, 10, 100, 5, 0.025, SEED, _lib.MODE["serial"])   # CSE on two tables
    assert rc == _lib.ESTATE and b"four tables" in _lib.lib.smore_last_error(pn.ctx)
    with pytest.raises(SmoreError, match="table not allocated"):
        pn.get_table(2)
    pn.LoadEdgeList(os.path.join(GOLDEN, "bip.txt"), 1)   # a new graph drops the fields
    pn.alloc_tables(8, 4)
    with pytest.raises(SmoreError, match="no fields"):
        pn.train_cse(0, 0, 10, 100, 5, 0.025, SEED, "serial")
    with pytest.raises(SmoreError, match="no fields"):
        pn.cse_records(1, 0, 10, 5, SEED)
    f = np.ones(pn.MAX_vid, np.int32)
    pn.set_fields(f, 2)
    rc = _lib.lib.smore_train_cse(pn.ctx, 0, 0, 10, 100, 5, 0.025, SEED, _lib.MODE["serial"])
    assert rc == _lib.ESTATE and b"source mass" in _lib.lib.smore_last_error(pn.ctx)
    pn.LoadFieldMeta(os.path.join(GOLDEN, "bip_field.txt"))
    for bad in (-1, 4):
        rc = _lib.lib.smore_train_cse(pn.ctx, 0, 0, 10, 100, 5, 0.025, SEED, bad)
        assert rc == _lib.EINVAL and b"bad mode" in _lib.lib.smore_last_error(pn.ctx)
    for steps in (0, 11):
        rc = _lib.lib.smore_train_cse(pn.ctx, 1, 0, 10, 100, steps, 0.025, SEED, _lib.MODE["serial"])
        assert rc == _lib.EINVAL and b"walk_steps" in _lib.lib.smore_last_error(pn.ctx)
    rc = _lib.lib.smore_train_cse(pn.ctx, 2, 0, 10, 100, 5, 0.025, SEED, _lib.MODE["serial"])
    assert rc == _lib.EINVAL and b"rank" in _lib.lib.smore_last_error(pn.ctx)
    rc = _lib.lib.smore_train_cse(pn.ctx, 1, 0, 10, 100, 5, 0.025, SEED, _lib.MODE["hogwild"])
    assert rc == _lib.EINVAL and b"plain-store" in _lib.lib.smore_last_error(pn.ctx)
    # every training entry that is not CSE refuses the four-table context
    L = _lib.lib
    m = _lib.MODE["atomic"]
    calls = [lambda: L.smore_train_edges(pn.ctx, _lib.MODEL["line2"], 0, 10, 100, 5, 0.025, 0.0, SEED, m),
             lambda: L.smore_train_hoprec(pn.ctx, 0, 10, 100, 5, 0.025, SEED, m),
             lambda: L.smore_train_warp(pn.ctx, 0, 10, 100, 0.025, SEED, m),
             lambda: L.smore_train_hpe(pn.ctx, 0, 10, 100, 3, 5, 0.01, 0.025, SEED, m),
             lambda: L.smore_census_begin(pn.ctx),
             lambda: L.smore_set_hot_threshold(pn.ctx, 0.5),
             lambda: L.smore_block_setup(pn.ctx, _lib.MODEL["line2"], 1, 0, 5, m),
             lambda: L.smore_exchange_begin(pn.ctx, 1)]
    for k, call in enumerate(calls):
        assert call() == _lib.ESTATE, k
        assert b"four-table" in L.smore_last_error(pn.ctx), k
    pn.set_semantics("go")
    with pytest.raises(SmoreError, match="Go semantics"):
        pn.train_cse(0, 0, 10, 100, 5, 0.025, SEED, "serial")
    pn.set_semantics("cpp")
    pn.train_cse(1, 0, 10, 100, 5, 0.025, SEED, "serial")   # and now it runs
    assert pn.cse_stats()[0] >= 10


# ---------------------------------------------------------------- model class and CLI
E2E_SAMPLES = 100000   # of the fixtures' 10^6: the full run in serial would take most of a minute


def saved_text(names, field, T, dim):
    """NEMF::SaveWeights: WU rows for field 0, WI rows for field 1, else the name alone (%g)."""
    out = ["%d %d\n" % (len(names), dim)]
    for v, name in enumerate(names):
        row = T[cs.WU][v] if field[v] == 0 else T[cs.WI][v] if field[v] == 1 else []
        out.append(name + "".join(" %g" % float(x) for x in row[:dim]) + "\n")
    return "".join(out)


@pytest.fixture(scope="module")
def run_spec32():
    out = {}
    g = cs.graph("bip.txt")
    for rank in RANKS:
        z = cs.gold("e2e_%s_bip" % cs.RANKS[rank])
        dim, st, steps, seed = (int(x) for x in z["meta"])
        T = cs.pad4([z[k + "0"] for k in ("WU", "WI", "CU", "CI")], dim)
        r = cs.run(g, z["field"], T, steps, rank, float(z["meta_f"][0]), st * 10 ** 6, 0, E2E_SAMPLES, seed)
        out[rank] = (z, [t[:, :dim] for t in T], (r.tested, r.updated), saved_text(g.names, z["field"], T, dim))
    return out


@pytest.mark.parametrize("rank", RANKS)
def test_model_class_vs_fp32_spec(smore, run_spec32, capsys, tmp_path, rank):
    z, want, stats, text = run_spec32[rank]
    dim, st, steps, seed = (int(x) for x in z["meta"])
    m = (smore.NERANK if rank else smore.NEMF)(0, "serial", seed)
    assert (m.pnet.vertex_method, m.pnet.negative_method) == ("out_degrees", "degrees")
    m.LoadEdgeList(os.path.join(GOLDEN, "bip.txt"), 1)
    m.LoadFieldMeta(os.path.join(GOLDEN, "bip_field.txt"))
    m.Init(dim)
    for k, name in enumerate(("WU0", "WI0", "CU0", "CI0")):   # the reference's own Init
        np.testing.assert_array_equal(m.pnet.get_table(k), z[name].astype(np.float32))
    m.Train(st, steps, float(z["meta_f"][0]), 1, stop_after=E2E_SAMPLES)
    out = capsys.readouterr().out
    assert "[%s]" % cs.RANKS[rank].upper() in out and "walk steps:" in out and "Progress: 10.000 %" in out
    for k in range(4):
        np.testing.assert_array_equal(m.pnet.get_table(k), want[k], err_msg="table %d" % k)
    assert m.pnet.cse_stats() == stats
    path = str(tmp_path / "rep.txt")
    m.SaveWeights(path)
    assert open(path).read() == text


@pytest.mark.parametrize("rank", RANKS)
def test_cli_vs_fp32_spec(run_spec32, tmp_path, rank):
    z, _want, _stats, text = run_spec32[rank]
    dim, st, steps, seed = (int(x) for x in z["meta"])
    out = str(tmp_path / "rep.txt")
    r = subprocess.run([os.path.join(BIN, cs.RANKS[rank]), "-train", os.path.join(GOLDEN, "bip.txt"), "-field",
                        os.path.join(GOLDEN, "bip_field.txt"), "-save", out, "-dimensions", str(dim),
                        "-sample_times", str(st), "-walk_steps", str(steps), "-alpha", "0.025", "-threads", "1",
                        "-seed", str(seed), "-mode", "serial", "-stop_after", str(E2E_SAMPLES)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for heading in ("Connections:", "Meta Data Preview:", "# of meta data:\t\t295", "# of field:\t\t2", "Model Setting:",
                    "[%s]" % cs.RANKS[rank].upper(), "Learning Parameters:", "walk steps:\t\t5", "Start Training[1]:",
                    "Save Model:", "Save to <"):
        assert heading in r.stdout, heading
    assert open(out).read() == text


def test_save_weights_fields_names_only_for_other_fields(smore, tmp_path):
    g, field, pn = make_pair(smore, "pl3")   # three fields: the third gets its name alone
    pn.alloc_tables(5, 4)
    pn.init_tables_glibc_pair(0, 1, 0)
    path = str(tmp_path / "rep.txt")
    pn.save_weights_fields([0, 1, -1], path)
    assert open(path).read() == saved_text(g.names, field, get(pn), 5)
    assert any(len(ln.split()) == 1 for ln in open(path).read().splitlines()[1:])


def test_cli_usage_and_gpus():
    for prog in ("nemf", "nerank"):
        r = subprocess.run([os.path.join(BIN, prog)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "Usage:" in r.stdout and "-field" in r.stdout and "-walk_steps" in r.stdout
        r = subprocess.run([os.path.join(BIN, prog), "-train", os.path.join(GOLDEN, "bip.txt"), "-field",
                            os.path.join(GOLDEN, "bip_field.txt"), "-save", "/dev/null", "-gpus", "2"],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "one GPU" in r.stderr
