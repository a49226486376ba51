#!/usr/bin/env python3
"""Throughput of the other configs of BASELINE.json on one MI355X (the
headline LINE-2 C4 number is bench.py's).  One JSON line per config:

  c2   LINE order 2, 1M vertices / 20M lines, d=64, K=5   (M edge-updates/s)
  c4   LINE order 2, 10M vertices / 200M lines (bench.py's headline config)
  c3   BPR (C++ rule: 5 rounds per sample), 2M users x 1M items / 100M edges,
       d=128, negatives uniform over items (BPR's "no_degrees")   (M BPR samples/s)
  c5   DeepWalk, Youtube-links-sized stand-in (1.13M vertices / 3M lines),
       d=128, walk_steps=40, window=5, K=5 (M skip-gram pair-updates/s, from the
       exact pairs-per-walk expectation of the window-shrink rule)

Timing: HIP events of the library (smore_last_kernel_ms) over `--steps`
calls after one warmup call, inputs resident in HBM.

    python tools/bench_models.py --configs c2 c3 c5 [--mode hybrid]
  c5go / c5n2v  Go DeepWalk / Go node2vec (p 0.5, q 2) on c5's graph
  warp WARP on c3's graph, d=128 (M WARP samples/s, and the mean trials per
       sample from smore_warp_stats; "hybrid" runs the atomic scatter)
  hoprec HOP-REC on c3's graph loaded undirected, d=128, walk_steps 5, fields
       from the generator's user / item split (M HOP-REC samples/s, the gates
       passed per sample from smore_hoprec_stats, draw / update ms; "hybrid"
       runs the atomic scatter, there is no plain-store one)
  skewopt Skew-OPT on c3's graph, d=128, defaults xi 10 / omega 3 / eta 3 from
       SPR::Init's table (M Skew-OPT samples/s and M rows/s: 18 rows read per
       sample plus the rows written, from smore_skewopt_stats; "hybrid" runs
       the atomic scatter, there is no plain-store one)
  cse  CSE (nemf, then nerank) on c3's graph loaded undirected, d=128,
       walk_steps 5, fields from the generator's user / item split, NEMF::Init's
       tables (M CSE samples/s and M rows/s: per sample 2 + 12 walk_steps rows
       read and added, plus nemf's 5 read and added or nerank's 8 or 16 read
       and its one added when a gate passes; draw / update ms; "hybrid" runs the atomic scatter, there is no
       plain-store one)
  cbow GCN, then TEXTGCN (the set-sum rule) on c3's graph loaded undirected,
       d=128, walk_steps 5, negative_samples 5, reg 0.01, fields from the
       generator's user / item split, GCN::Init's table (M CBOW samples/s and
       M rows/s: per sample 2 S + K S rows read and as many added, 70 at the
       defaults; draw / update ms; clean share from smore_cbow_stats; "hybrid"
       runs the atomic scatter, there is no plain-store one)
  eco  ECO (the sampled-softmax choice rule) on c3's graph loaded undirected,
       d=128, negative_samples 5, reg 0.01, fields from the generator's user /
       item split, uniform negatives, ECO::Init's table (M ECO samples/s and M
       rows/s: per sample 1 + 5 (2 + K) rows read and as many added, 72 at the
       defaults; draw / update ms; clean share from smore_eco_stats; "hybrid"
       runs the atomic scatter, there is no plain-store one)
  textgcndev TEXTGCNdev (the bag-of-words event rule) on c3's graph loaded
       undirected, d=128, num_events 1, num_words 5, reg 0.01, fields from the
       generator's user / item split, TEXTGCNdev::Init's tables (M CBOWdev
       samples/s and M rows/s: per sample 2 + E N + 10 E rows read and as many
       added, 17 and 17 at the defaults; draw / update ms; clean share from
       smore_cbowdev_stats; "hybrid" runs the atomic scatter, there is no
       plain-store one)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pairs_per_walk(L, window):
    """E[# (i, j) pairs] of SkipGrams with the random shrink r ~ U{1..w}
    (src/proNet.cpp:769-809) on a walk of L vertices."""
    tot = 0.0
    for i in range(L):
        for r in range(1, window + 1):
            lo, hi = max(0, i - r), min(L - 1, i + r)
            tot += (hi - lo) / window
    return tot


def ran(pn):
    """The scatter the last call actually ran (smore_last_mode): "plain" for
    the plain-store kernel (C++ BPR's hybrid above the small-graph cap)."""
    m = pn.last_mode()
    return "plain" if m == "hogwild" else m


def run_edges(pn, model, S, steps, K, mode, seed=7):
    """mean ms per call, and the mean (draw, update) phase ms"""
    total = (steps + 1) * S
    ms, ph = [], []
    for k in range(steps + 1):
        pn.train_edges(model, k * S, S, total, K, 0.025, 0.0, seed, mode)
        if k:
            ms.append(pn.last_kernel_ms())
            ph.append(pn.last_phase_ms()[:2])
    return float(np.mean(ms)), [round(float(x), 3) for x in np.mean(ph, axis=0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c2", "c3", "c5"])
    ap.add_argument("--mode", default="hybrid")
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    import smore_amd
    from smore_amd import graphgen
    for cfg in args.configs:
        V, (src, dst, w) = graphgen.config_edges("c5" if cfg.startswith("c5") else "c3" if cfg in ("warp", "hoprec", "skewopt", "cse", "cbow", "eco", "textgcndev") else cfg)
        pn = smore_amd.ProNet(0)
        t0 = time.perf_counter()
        if cfg in ("c3", "warp", "hoprec", "skewopt", "eco"):
            pn.SetNegativeMethod("no_degrees")       # BPR() / WARP() / HBPR() / SPR() / ECO() (src/model/BPR.cpp:4-7, WARP.cpp:4-7)
        if cfg in ("hoprec", "cse", "cbow", "eco", "textgcndev"):
            # HBPR, NEMF, NERANK, GCN and TEXTGCN load undirected (cli/hoprec.cpp:63, cli/nemf.cpp, cli/gcn.cpp): every line also as item -> user
            users = int(src.max()) + 1               # the generator's split: users [0, users), items after them
            assert int(dst.min()) >= users
            src, dst, w = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([w, w])
        pn.set_graph_edges(V, src, dst, w)
        build = time.perf_counter() - t0
        out = {"config": cfg, "vertices": V, "edge_slots": pn.MAX_line, "mode": args.mode,
               "build_s": round(build, 1)}
        if cfg in ("c2", "c4"):
            S = 1 << 27
            pn.alloc_tables(64, 2)
            pn.init_table_uniform(0, 1)
            pn.zero_table(1)
            ms, ph = run_edges(pn, "line2", S, args.steps, 5, args.mode)
            out.update(model="line2", dim=64, K=5, samples_per_call=S, ms_per_call=round(ms, 3),
                       draw_update_ms=ph, value=round(S / ms / 1e3, 1), unit="M edge-updates/s")
        elif cfg == "c3":
            S = 1 << 26
            pn.alloc_tables(128, 1)
            pn.init_table_uniform(0, 1)
            ms, ph = run_edges(pn, "bpr", S, args.steps, 5, args.mode)
            out.update(model="bpr", dim=128, rounds=5, samples_per_call=S, ms_per_call=round(ms, 3),
                       draw_update_ms=ph,
                       value=round(S / ms / 1e3, 1), unit="M BPR samples/s (5 rounds each)")
        elif cfg == "warp":
            S = 1 << 26
            pn.alloc_tables(128, 1)
            pn.init_table_uniform(0, 1)
            total = (args.steps + 1) * S
            ms, ph, st = [], [], []
            for k in range(args.steps + 1):
                pn.train_warp(k * S, S, total, 0.025, 7, args.mode)
                st.append(pn.warp_stats())
                if k:
                    ms.append(pn.last_kernel_ms())
                    ph.append(pn.last_phase_ms()[:2])
            ms = float(np.mean(ms))
            out.update(model="warp", dim=128, samples_per_call=S, ms_per_call=round(ms, 3),
                       draw_update_ms=[round(float(x), 3) for x in np.mean(ph, axis=0)],
                       trials_per_sample=round((st[-1][0] - st[0][0]) / (args.steps * S), 4),
                       updated_per_sample=round((st[-1][1] - st[0][1]) / (args.steps * S), 4),
                       value=round(S / ms / 1e3, 1), unit="M WARP samples/s")
        elif cfg == "hoprec":
            S, walk_steps = 1 << 24, 5
            pn.set_fields((np.arange(V) >= users).astype(np.int32), 2)
            pn.alloc_tables(128, 1)
            pn.init_table_uniform(0, 1)
            total = (args.steps + 1) * S
            ms, ph, st = [], [], []
            for k in range(args.steps + 1):
                pn.train_hoprec(k * S, S, total, walk_steps, 0.025, 7, args.mode)
                st.append(pn.hoprec_stats())
                if k:
                    ms.append(pn.last_kernel_ms())
                    ph.append(pn.last_phase_ms()[:2])
            ms = float(np.mean(ms))
            out.update(model="hoprec", dim=128, walk_steps=walk_steps, samples_per_call=S, ms_per_call=round(ms, 3),
                       draw_update_ms=[round(float(x), 3) for x in np.mean(ph, axis=0)],
                       gates_passed_per_sample=round((st[-1][1] - st[0][1]) / (args.steps * S), 4),
                       skipped=pn.skipped(),
                       value=round(S / ms / 1e3, 2), unit="M HOP-REC samples/s")
        elif cfg == "cse":
            S, walk_steps = 1 << 24, 5
            pn.set_fields((np.arange(V) >= users).astype(np.int32), 2)
            for rank, name in enumerate(("nemf", "nerank")):
                pn.alloc_tables(128, 4)
                pn.init_tables_glibc_pair(0, 1, 0)   # NEMF::Init
                total = (args.steps + 1) * S
                ms, ph, st = [], [], []
                for k in range(args.steps + 1):
                    pn.train_cse(rank, k * S, S, total, walk_steps, 0.025, 7, args.mode)
                    st.append(pn.cse_stats())
                    if k:
                        ms.append(pn.last_kernel_ms())
                        ph.append(pn.last_phase_ms()[:2])
                ms = float(np.mean(ms))
                tested = (st[-1][0] - st[0][0]) / (args.steps * S)
                updated = (st[-1][1] - st[0][1]) / (args.steps * S)
                # rows moved per sample: WU[v], WI[c] and 12 context rows per step read and added; the
                # direct term reads 5 and adds 5 (nemf), or reads batches of 8 (an upper estimate from
                # the mean gates tested) and adds the one negative that passes (nerank)
                rows = 2 * (2 + 12 * walk_steps) + (8 * np.ceil(max(tested, 1.0) / 8) + updated if rank else 10)
                res = dict(out, model=name, dim=128, walk_steps=walk_steps, samples_per_call=S, ms_per_call=round(ms, 3),
                           draw_update_ms=[round(float(x), 3) for x in np.mean(ph, axis=0)],
                           gates_tested_per_sample=round(tested, 4),
                           updated_per_sample=round(updated, 4), rows_per_sample=round(float(rows), 2),
                           skipped=pn.skipped(), rows_per_s_M=round(S * rows / ms / 1e3, 1), scatter=ran(pn),
                           value=round(S / ms / 1e3, 2), unit="M CSE samples/s")
                print(json.dumps(res), flush=True)
            pn.close()
            continue
        elif cfg == "cbow":
            S, ws, K = 1 << 24, 5, 5
            pn.set_fields((np.arange(V) >= users).astype(np.int32), 2)
            for model, name in enumerate(("gcn", "textgcn")):
                pn.alloc_tables(128, 1)
                pn.init_table_glibc(0, 0)   # GCN::Init's w_vertex
                total = (args.steps + 1) * S
                ms, ph, st = [], [], []
                for k in range(args.steps + 1):
                    pn.train_cbow(model, k * S, S, total, ws, K, 0.025, 0.01, 7, args.mode)
                    st.append(pn.cbow_stats())
                    if k:
                        ms.append(pn.last_kernel_ms())
                        ph.append(pn.last_phase_ms()[:2])
                ms = float(np.mean(ms))
                clean = (st[-1][0] - st[0][0]) / (args.steps * S)
                # rows moved per sample: every row of the 2 + K sets is read once and added to once
                rows = 2 * (2 * ws + K * ws)
                res = dict(out, model=name, dim=128, walk_steps=ws, negative_samples=K, samples_per_call=S,
                           ms_per_call=round(ms, 3), draw_update_ms=[round(float(x), 3) for x in np.mean(ph, axis=0)],
                           clean_share=round(clean, 4), rows_per_sample=rows, skipped=pn.skipped(),
                           rows_per_s_M=round(S * rows / ms / 1e3, 1), scatter=ran(pn),
                           value=round(S / ms / 1e3, 2), unit="M CBOW samples/s")
                print(json.dumps(res), flush=True)
            pn.close()
            continue
        elif cfg == "eco":
            S, K = 1 << 24, 5
            pn.set_fields((np.arange(V) >= users).astype(np.int32), 2)
            pn.alloc_tables(128, 1)
            pn.init_table_glibc_unscaled(0, 0, 2)   # ECO::Init's w_vertex
            total = (args.steps + 1) * S
            ms, ph, st = [], [], []
            for k in range(args.steps + 1):
                pn.train_eco(k * S, S, total, K, 0.025, 0.01, 7, args.mode)
                st.append(pn.eco_stats())
                if k:
                    ms.append(pn.last_kernel_ms())
                    ph.append(pn.last_phase_ms()[:2])
            ms = float(np.mean(ms))
            clean = (st[-1][0] - st[0][0]) / (args.steps * S)
            # rows moved per sample: W[v] and every row of the five lists is read once and added to once
            rows = 2 * (1 + 5 * (2 + K))
            res = dict(out, model="eco", dim=128, negative_samples=K, samples_per_call=S, ms_per_call=round(ms, 3),
                       draw_update_ms=[round(float(x), 3) for x in np.mean(ph, axis=0)], clean_share=round(clean, 4),
                       rows_per_sample=rows, skipped=pn.skipped(), finite=bool(np.isfinite(pn.get_table(0)).all()),
                       rows_per_s_M=round(S * rows / ms / 1e3, 1), scatter=ran(pn),
                       value=round(S / ms / 1e3, 2), unit="M ECO samples/s")
            print(json.dumps(res), flush=True)
            pn.close()
            continue
        elif cfg == "textgcndev":
            S, E, N = 1 << 24, 1, 5
            pn.set_fields((np.arange(V) >= users).astype(np.int32), 2)
            pn.alloc_tables(128, 2)
            pn.init_table_glibc(0, 0)          # TEXTGCNdev::Init: w_vertex whole, then w_context
            pn.init_table_glibc(1, V * 128)
            total = (args.steps + 1) * S
            ms, ph, st = [], [], []
            for k in range(args.steps + 1):
                pn.train_cbowdev(k * S, S, total, E, N, 0.025, 0.01, 7, args.mode)
                st.append(pn.cbowdev_stats())
                if k:
                    ms.append(pn.last_kernel_ms())
                    ph.append(pn.last_phase_ms()[:2])
            ms = float(np.mean(ms))
            clean = (st[-1][0] - st[0][0]) / (args.steps * S)
            # rows moved per sample: user, event, the bag and the negatives are read once and added to
            # once (the event row takes 2 E adds on one read)
            rows = 2 * (2 + E * N + 10 * E)
            res = dict(out, model="textgcndev", dim=128, num_events=E, num_words=N, samples_per_call=S,
                       ms_per_call=round(ms, 3), draw_update_ms=[round(float(x), 3) for x in np.mean(ph, axis=0)],
                       clean_share=round(clean, 4), rows_per_sample=rows, skipped=pn.skipped(),
                       finite=bool(np.isfinite(pn.get_table(0)).all() and np.isfinite(pn.get_table(1)).all()),
                       rows_per_s_M=round(S * rows / ms / 1e3, 1), scatter=ran(pn),
                       value=round(S / ms / 1e3, 2), unit="M CBOWdev samples/s")
            print(json.dumps(res), flush=True)
            pn.close()
            continue
        elif cfg == "skewopt":
            S = 1 << 24
            pn.alloc_tables(128, 1)
            pn.init_table_glibc_offset(0, 0, 0.01)   # SPR::Init
            total = (args.steps + 1) * S
            ms, ph, st = [], [], []
            for k in range(args.steps + 1):
                pn.train_skewopt(k * S, S, total, 0.025, 10.0, 3.0, 3, 7, args.mode)
                st.append(pn.skewopt_stats())
                if k:
                    ms.append(pn.last_kernel_ms())
                    ph.append(pn.last_phase_ms()[:2])
            ms = float(np.mean(ms))
            passed = (st[-1][0] - st[0][0]) / (args.steps * S)
            updated = (st[-1][1] - st[0][1]) / (args.steps * S)
            # rows moved per sample: 18 read; written: the passed negatives and, when any passed, i and v
            out.update(model="skewopt", dim=128, samples_per_call=S, ms_per_call=round(ms, 3),
                       draw_update_ms=[round(float(x), 3) for x in np.mean(ph, axis=0)],
                       gates_passed_per_sample=round(passed, 4), updated_per_sample=round(updated, 4),
                       skipped=pn.skipped(), rows_per_s_M=round(S * (18 + passed + 2 * updated) / ms / 1e3, 1),
                       value=round(S / ms / 1e3, 2), unit="M Skew-OPT samples/s")
        elif cfg == "c5":
            steps_, window, K, walk_times = 40, 5, 5, 1
            pn.alloc_tables(128, 2)
            pn.init_table_uniform(0, 1)
            pn.init_table_uniform(1, 2)
            order = smore_amd.deepwalk_order(V, walk_times + 1, 0)
            ms = []
            for k in range(args.steps + 1):
                pn.train_deepwalk(0, V, walk_times + 1, steps_, window, K, 0.025, 7 + k, order, args.mode)
                if k:
                    ms.append(pn.last_kernel_ms())
            ms = float(np.mean(ms))
            ppw = pairs_per_walk(steps_ + 1, window)
            out.update(model="deepwalk", dim=128, K=K, walk_steps=steps_, window=window, walks_per_call=V,
                       ms_per_call=round(ms, 3), pairs_per_walk=round(ppw, 1),
                       value=round(V * ppw / ms / 1e3, 1), unit="M pair-updates/s",
                       walks_per_s=round(V / ms * 1e3, 1))
        elif cfg in ("c5go", "c5n2v"):
            # Go DeepWalk / Go node2vec (p=0.5, q=2) on C5's graph, --mode scatter
            steps_, window, K = 40, 5, 5
            pn.set_semantics("go")
            pn.alloc_tables(128, 2)
            pn.init_table_uniform(0, 1)
            pn.init_table_uniform(1, 2)
            order = smore_amd.deepwalk_order(V, 2, 0)
            ms = []
            for k in range(args.steps + 1):
                if cfg == "c5go":
                    pn.train_deepwalk(0, V, 2, steps_, window, K, 0.025, 7 + k, order, args.mode)
                else:
                    pn.train_node2vec(0, V, 2, steps_, window, K, 0.025, 0.5, 2.0, 7 + k, order, args.mode)
                if k:
                    ms.append(pn.last_kernel_ms())
            ms = float(np.mean(ms))
            L = steps_ + 1
            ppw = sum(min(i + window, L - 1) - max(i - window, 0) for i in range(L))   # Go fixed window
            out.update(model="go_deepwalk" if cfg == "c5go" else "go_node2vec", dim=128, K=K, walk_steps=steps_,
                       window=window, walks_per_call=V, ms_per_call=round(ms, 3), pairs_per_walk=ppw,
                       value=round(V * ppw / ms / 1e3, 1), unit="M pair-updates/s",
                       walks_per_s=round(V / ms * 1e3, 1))
        out["scatter"] = ran(pn)       # what ran; "mode" is what was asked for
        print(json.dumps(out), flush=True)
        pn.close()


if __name__ == "__main__":
    main()
