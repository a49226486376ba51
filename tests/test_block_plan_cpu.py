"""The block schedule's host-only plan (smore_amd/csrc/block_plan.cpp: what
smore_block_setup computes before it touches the device) run on the CPU by
tests/c/block_plan_check and compared, table by table, with its numpy
restatement tests/block_spec.py.  Needs no GPU."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from tests.block_spec import BlockSpec, hub_count, part_masses, prob_thr, skewed_graph_lines
from tests.conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "tests", "c", "block_plan_check")
PL1K = os.path.join(GOLDEN, "pl1k.txt")
K = 5
ID = 0x3FFFFFFF
DTYPE = {"i64": np.int64, "u64": np.uint64, "f64": np.float64, "i32": np.int32, "u32": np.uint32, "u8": np.uint8}


def _plan(out, path, und, model, nparts, part, H, hybrid=0, M=0, tau=0.0):
    out.mkdir(exist_ok=True)
    r = subprocess.run([BIN, path, str(und), model, str(nparts), str(part), str(K), str(H), str(hybrid), str(M),
                        repr(tau), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    plan = {}
    for entry in (out / "index.txt").read_text().split():
        name, typ, n = entry.split(":")
        plan[name] = np.fromfile(str(out / (name + ".bin")), DTYPE[typ])
        assert len(plan[name]) == int(n)
    return plan


@pytest.fixture(scope="module")
def graph():
    return orc.Graph.from_file(PL1K, 1)


def test_block_plan_binary_built():
    assert os.access(BIN, os.X_OK), "build it with `make plan_check`"


def _check_atom_table(words, atoms, tab):
    """An alias table over `atoms` [(v, c, w)] in the device layout: {thr, v,
    c, 0}, {v', c', 0, 0} per atom, (v', c') the alias atom's; no tags."""
    v = np.array([a[0] for a in atoms], np.uint32)
    c = np.array([a[1] for a in atoms], np.uint32)
    thr, al = tab
    want = np.zeros((len(atoms), 8), np.uint32)
    want[:, 0], want[:, 1], want[:, 2], want[:, 4], want[:, 5] = thr, v, c, v[al], c[al]
    np.testing.assert_array_equal(words, want)


@pytest.mark.parametrize("n,hubs", [(2, -1), (3, -1), (4, -1), (8, -1), (2, 0), (4, 0), (3, 100)])
def test_plan_tables_match_spec(tmp_path, graph, n, hubs):
    """Every table of every part against the spec, LINE-2, not hybrid: 2 parts
    with no hubs, 8 parts with the automatic hubs, 100 hubs on the 920-vertex
    graph."""
    nb = 2 * n
    H = hub_count(graph.V, nb, hubs)
    for r in range(n):
        spec = BlockSpec(graph, n, r, K, hubs)
        p = _plan(tmp_path / ("p%d" % r), PL1K, 1, "line2", n, r, H)
        assert spec.H == H
        assert list(p["wb"]) == spec.wb and list(p["cb"]) == spec.cb and list(p["hubs"]) == spec.hubs
        off = [0]
        for a in spec.atoms + ([spec.hub_atoms] if H else []):
            off.append(off[-1] + len(a))
        assert list(p["atom_off"]) == off
        ntab = p["ntab"].reshape(-1, 2)
        np.testing.assert_array_equal(ntab[:, 0], spec.nthr)
        np.testing.assert_array_equal(ntab[:, 1].view(np.int32), spec.nal)
        hnt = p["hub_ntab"].reshape(-1, 2)
        np.testing.assert_array_equal(hnt[:, 0], spec.hthr)
        np.testing.assert_array_equal(hnt[:, 1].view(np.int32), spec.hal)
        words = p["atoms"].reshape(-1, 8)
        assert len(words) == off[-1]
        for k in range(nb):
            if spec.atoms[k]:
                _check_atom_table(words[off[k]:off[k + 1]], spec.atoms[k], spec.tabs[k])
        hub_off, nhub = (int(x) for x in p["hub_range"])
        assert nhub == len(spec.hub_atoms) and (hub_off == off[nb] if H else nhub == 0)
        if spec.hub_atoms:
            _check_atom_table(words[hub_off:hub_off + nhub], spec.hub_atoms, spec.hub_tab)
        np.testing.assert_allclose(p["mass"], spec.mass, rtol=1e-12, atol=0)
        np.testing.assert_allclose(p["nmass"], spec.nmass, rtol=1e-12, atol=0)
        pm, _ = part_masses(PL1K, n)
        np.testing.assert_allclose(p["part_mass"], pm, rtol=1e-12, atol=0)
        assert [prob_thr(x) for x in p["hub_p"]] == spec.hub_thr


@pytest.mark.parametrize("n", [2, 4, 8])
def test_plan_part_mass_on_the_skewed_graph(tmp_path, n):
    """The product's W parts and part masses on the graph of
    test_blocks_cpu.py::test_part_mass_split_on_a_skewed_graph."""
    f = tmp_path / "skewed.txt"
    f.write_text(skewed_graph_lines())
    pm, wb = part_masses(str(f), n, undirected=0)
    p = _plan(tmp_path / "p", str(f), 0, "line2", n, 0, 0)
    assert list(p["wb"]) == wb
    np.testing.assert_allclose(p["part_mass"], pm, rtol=1e-12, atol=0)
    assert max(p["part_mass"]) > 1.1 / n


@pytest.mark.parametrize("n", [2, 4])
def test_plan_walk_cells_share_the_line2_laws(tmp_path, graph, n):
    """Walk cells cut the graph by the same laws as LINE-2 cells: bounds, hubs,
    negative masses and negative tables equal; hub_of inverts hubs.  100 hubs
    (the automatic rule gives none at 2 and 4 parts)."""
    H = 100
    for r in range(n):
        a = _plan(tmp_path / ("l%d" % r), PL1K, 1, "line2", n, r, H)
        b = _plan(tmp_path / ("w%d" % r), PL1K, 1, "walk", n, r, H)
        for name in ("wb", "cb", "hubs", "hub_rate", "nmass", "part_mass", "ntab", "hub_ntab"):
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)
        assert len(b["atoms"]) == 0 and not b["atom_off"].any()
        want = np.full(graph.V, -1, np.int32)
        want[b["hubs"]] = np.arange(H)
        np.testing.assert_array_equal(b["hub_of"], want)
        assert len(a["hub_of"]) == 0


TAG_M, TAG_TAU = 16, 0.3


def test_plan_hot_tags_are_consistent(tmp_path, graph):
    """The hybrid plan's hot tags (bits 30 / 31 of the table words), pl1k, 4
    parts, 100 hubs, M = 16 resident groups, tau = 0.3: chosen on the CPU so
    that both kinds occur -- summed over the 4 parts' 8 cells each, 2622 hot
    and 1058 cold block C rows, 202 hot and 7158 cold W rows, 177 hot and 223
    cold hub slots (M = 64 makes every slot hot, M = 2 every block row cold).

    Within a cell every table entry naming a C row carries that row's one
    tag, the cell's flag M p > tau of its law; a hub slot's tag is the same in
    every cell (hot in any); a W row's tag in a cell's atom table is the
    cell's (M times its share of the cell's atom mass > tau, recomputed here
    from the spec's atoms in the product's order), and in the hub atom table
    the OR over the cells."""
    n, H, M, tau = 4, 100, TAG_M, TAG_TAU
    nb, V = 2 * n, graph.V
    seen = {"c_hot": 0, "c_cold": 0, "w_hot": 0, "w_cold": 0, "slot_hot": 0, "slot_cold": 0}
    for r in range(n):
        spec = BlockSpec(graph, n, r, K, H)
        p = _plan(tmp_path / ("p%d" % r), PL1K, 1, "line2", n, r, H, 1, M, tau)
        cb, wlo, whi = p["cb"], spec.wb[r], spec.wb[r + 1]
        ends = np.cumsum([cb[k + 1] - cb[k] + H for k in range(nb)])
        pcb, hcb = np.split(p["pcb"], ends[:-1]), np.split(p["hcb"], ends[:-1])
        ntab, hnt = p["ntab"].reshape(-1, 2), p["hub_ntab"].reshape(-1, 2)
        words = p["atoms"].reshape(-1, 8)
        off = p["atom_off"]
        # the C flags: a block row's from its cell's law, a slot's hot in any cell
        slot_hot = np.zeros(H, bool)
        for k in range(nb):
            rows = cb[k + 1] - cb[k]
            np.testing.assert_array_equal(hcb[k][:rows] != 0, M * pcb[k][:rows] > tau)
            slot_hot |= M * pcb[k][rows:] > tau
        mH = 0.0
        for _, _, w in spec.hub_atoms:
            mH += w
        w_any = np.zeros(whi - wlo, bool)
        for k in range(nb):
            lo, rows = int(cb[k]), int(cb[k + 1] - cb[k])
            np.testing.assert_array_equal(hcb[k][rows:] != 0, slot_hot)

            def c_tag(x):
                return hcb[k][x - lo] if x < V else hcb[k][rows + x - V]
            # negative entries: bit 31 the entry's own row, bit 30 its alias
            ent = np.concatenate([ntab[lo:lo + rows], hnt[k * H:(k + 1) * H]])
            ids = list(range(lo, lo + rows)) + list(range(V, V + H))
            for i, (_, al) in enumerate(ent):
                assert (int(al) >> 31) == c_tag(ids[i]) and ((int(al) >> 30) & 1) == c_tag(int(al) & ID)
            # the cell's W law, in the product's order of float sums
            pw = [0.0] * (whi - wlo)
            mraw = 0.0
            for v, _, w in spec.atoms[k]:
                pw[v - wlo] += w
                mraw += w
            for v, _, w in spec.hub_atoms:
                pw[v - wlo] += w / nb
            mraw += mH / nb
            w_hot = np.array([mraw > 0 and M * x / mraw > tau for x in pw])
            w_any |= w_hot
            t = words[off[k]:off[k + 1]]
            for col in (1, 4):
                np.testing.assert_array_equal(t[:, col] >> 30, w_hot[(t[:, col] & ID) - wlo])
            for col in (2, 5):
                assert (t[:, col] >> 30).tolist() == [c_tag(int(x)) for x in t[:, col] & ID]
            seen["c_hot"] += int(hcb[k][:rows].sum())
            seen["c_cold"] += int(rows - hcb[k][:rows].sum())
            seen["w_hot"] += int(w_hot.sum())
            seen["w_cold"] += int((~w_hot).sum())
        t = words[off[nb]:off[nb + 1]]
        for col in (1, 4):
            np.testing.assert_array_equal(t[:, col] >> 30, w_any[(t[:, col] & ID) - wlo])
        for col in (2, 5):
            np.testing.assert_array_equal(t[:, col] >> 30, slot_hot[(t[:, col] & ID) - V])
        seen["slot_hot"] += int(slot_hot.sum())
        seen["slot_cold"] += int((~slot_hot).sum())
    assert all(x > 0 for x in seen.values()), seen
