// block_plan.cpp -- the host-only plan of one part's block tables
// (block_plan.h): hub rows, W parts and C blocks, the mass vectors, this
// part's LINE-2 atoms bucketed by C block, the per-cell C-row laws and hot
// tags, and the negative and atom alias tables in their device layout.
// Every float loop runs in a fixed order (sequential per-bucket sums, atoms in
// vertex order), so the tables do not depend on the thread count.
#include "block_plan.h"

#include <algorithm>
#include <numeric>
#include <thread>

namespace smore {
namespace {

// f(k) for k in [0, n) on `threads` host threads (thread t: k = t, t + threads, ...)
template <class F>
void par_for(int n, int threads, F&& f) {
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            for (int k = t; k < n; k += threads) f(k);
        });
    for (auto& x : th) x.join();
}

// what the steps of one plan share besides the plan itself
struct Work {
    const HostGraph& g;
    const DrawLaws& law;
    const BlockPlanArgs& a;
    const int64_t V, H;
    const int nb, NBK;              // C blocks; atom buckets (+ 1 with hubs: the hub contexts')
    const int T;                    // host threads of the per-block passes
    int64_t wlo = 0, whi = 0;       // this part's W rows
    std::vector<int32_t> slot;      // with hubs: V entries, a hub's slot or -1
    double pnH = 0.0;               // the hubs' negative mass
    std::vector<double> nraw;       // per block: its raw negative mass (non-hub rows + 1/nb of the hubs')
    std::vector<int32_t> av, ac;    // LINE-2 atoms of this part, by bucket: source, context id
    std::vector<double> aw;         //   and mass
    std::vector<double> hubw;       // LINE-2: per hub slot, the part's atom mass of that context
    double mH = 0.0;                // LINE-2: the part's hub atom mass
    std::vector<std::vector<uint8_t>> hwb;   // LINE-2: per block, the hot flags of this part's W rows
    std::vector<uint8_t> hubhot, hwh;        // any-cell tags: per hub slot; per W row of the hub atoms

    Work(const HostGraph& g_, const DrawLaws& l, const BlockPlanArgs& a_)
        : g(g_), law(l), a(a_), V(g_.V), H(a_.H), nb(2 * a_.nparts), NBK(2 * a_.nparts + (a_.H > 0 ? 1 : 0)),
          T((int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), (unsigned)(2 * a_.nparts))) {}

    bool is_hub(int64_t x) const { return H > 0 && slot[x] >= 0; }
    // a C row's / this part's W row's hot tag in cell k (x >= V: a hub slot)
    uint32_t hc(const BlockPlan& p, int k, int64_t x) const {
        if (!a.hybrid) return 0u;
        if (x >= V) return hubhot[x - V];
        return p.hcb[k][x - p.cb[k]];
    }
    uint32_t hw(int k, int64_t v) const { return a.hybrid && !a.walk ? hwb[k][v - wlo] : 0u; }
};

// hub C rows: the H rows with the most expected touches per sample (as
// a positive context plus K times as a negative); slot j is row V + j
void pick_hubs(Work& w, BlockPlan& p) {
    const int64_t V = w.V, H = w.H;
    if (H <= 0) return;
    const std::vector<double>&pn = w.law.pn, &pc = w.law.pc;
    const int K = w.a.K;
    std::vector<int32_t> idx((size_t)V);
    std::iota(idx.begin(), idx.end(), 0);
    auto q = [&](int32_t x) { return pc[x] + (double)K * pn[x]; };
    std::partial_sort(idx.begin(), idx.begin() + H, idx.end(), [&](int32_t a, int32_t b) {
        return q(a) > q(b) || (q(a) == q(b) && a < b);
    });
    w.slot.assign((size_t)V, -1);
    p.hubs.assign(idx.begin(), idx.begin() + H);
    p.hub_rate.resize((size_t)H);
    for (int64_t j = 0; j < H; ++j) {
        w.slot[p.hubs[j]] = (int32_t)j;
        p.hub_rate[j] = q(p.hubs[j]);
        w.pnH += pn[p.hubs[j]];
    }
}

// W parts of equal source mass; C blocks of equal NON-hub negative mass (the
// hubs are in every block)
std::string cut_parts_and_blocks(Work& w, BlockPlan& p) {
    const int nparts = w.a.nparts;
    source_bounds(w.law.ps, nparts, p.wb);
    {
        std::vector<double> pcut = w.law.pn;
        for (int32_t x : p.hubs) pcut[x] = 0.0;
        source_bounds(pcut, w.nb, p.cb);
    }
    for (int q = 0; q < nparts; ++q)
        if (p.wb[q + 1] <= p.wb[q]) return "block schedule: an empty W part";
    for (int k = 0; k < w.nb; ++k)
        if (p.cb[k + 1] <= p.cb[k]) return "block schedule: an empty C block";
    w.wlo = p.wb[w.a.part];
    w.whi = p.wb[w.a.part + 1];
    return "";
}

void negative_and_part_mass(Work& w, BlockPlan& p) {
    const int nb = w.nb, nparts = w.a.nparts;
    const std::vector<double>&ps = w.law.ps, &pn = w.law.pn;
    // NegativeSample's share of each block: its non-hub rows, plus 1/nb of
    // every hub's (cell_args' negative weight)
    w.nraw.assign((size_t)nb, 0.0);
    {
        p.nmass.assign((size_t)nb, 0.0);
        double tot = 0.0;
        for (int k = 0; k < nb; ++k) {
            for (int64_t x = p.cb[k]; x < p.cb[k + 1]; ++x)
                if (!w.is_hub(x)) w.nraw[k] += pn[x];
            w.nraw[k] += w.pnH / nb;
            tot += w.nraw[k];
        }
        for (int k = 0; k < nb; ++k) p.nmass[k] = tot > 0 ? w.nraw[k] / tot : 1.0 / nb;
    }
    // each part's share of the source law: a round's samples are split over
    // the replicas by it (source_bounds only makes the parts roughly equal; a
    // hub above 1/N of the mass puts a part far off)
    {
        p.part_mass.assign((size_t)nparts, 0.0);
        double tot = 0.0;
        for (int q = 0; q < nparts; ++q) {
            for (int64_t v = p.wb[q]; v < p.wb[q + 1]; ++v) p.part_mass[q] += ps[v];
            tot += p.part_mass[q];
        }
        for (double& m : p.part_mass) m = tot > 0 ? m / tot : 1.0 / nparts;
    }
}

// LINE-2 atoms of this part: the TargetSample outcomes of its sources,
// bucketed by the context's block -- bucket nb: the hub contexts (as
// slot ids), shared by every block's cell
std::string bucket_atoms(Work& w, BlockPlan& p) {
    const HostGraph& g = w.g;
    const std::vector<double>& ps = w.law.ps;
    const int nb = w.nb, NBK = w.NBK;
    const int64_t V = w.V, wlo = w.wlo, whi = w.whi;
    auto bucket_of = [&](int64_t x) {
        if (w.is_hub(x)) return nb;
        return (int)(std::upper_bound(p.cb.begin(), p.cb.end(), x) - p.cb.begin()) - 1;
    };
    auto id_of = [&](int64_t x) { return w.is_hub(x) ? (int32_t)(V + w.slot[x]) : (int32_t)x; };
    // vertices [vb, ve) of the part, in order
    auto each_atom = [&](int64_t vb, int64_t ve, auto&& f) {
        for (int64_t v = vb; v < ve; ++v) {
            const int64_t off = g.offsets[v], br = g.offsets[v + 1] - off;
            if (br == 0 || ps[v] <= 0) continue;
            const double s = ps[v] / (double)br;
            for (int64_t i = 0; i < br; ++i) {
                const double pr = g.cprob[off + i];
                f(v, (int64_t)g.targets[off + i], s * pr);
                if (g.calias[off + i] >= 0 && pr < 1.0) f(v, g.calias[off + i], s * (1.0 - pr));
            }
        }
    };
    // two passes over vertex slices on every host thread (count per
    // (slice, bucket), then fill); the slices' order keeps each bucket's
    // atoms in vertex order, as one pass would
    const int TS = (int)std::max(1u, std::min(std::thread::hardware_concurrency(), 64u));
    std::vector<int64_t> vs((size_t)TS + 1);
    {   // slices of equal edge count
        const int64_t e0 = g.offsets[wlo], e1 = g.offsets[whi];
        for (int t = 0; t <= TS; ++t) {
            const int64_t e = e0 + (e1 - e0) * t / TS;
            vs[t] = t == 0 ? wlo : t == TS ? whi
                             : std::lower_bound(g.offsets.begin() + wlo, g.offsets.begin() + whi, e) -
                                   g.offsets.begin();
        }
    }
    std::vector<uint64_t> cnt((size_t)TS * NBK, 0);
    par_for(TS, TS, [&](int t) {
        uint64_t* ct = cnt.data() + (size_t)t * NBK;
        each_atom(vs[t], vs[t + 1], [&](int64_t, int64_t x, double m) {
            if (m > 0) ct[bucket_of(x)]++;
        });
    });
    std::vector<uint64_t> start((size_t)TS * NBK);
    for (int k = 0; k < NBK; ++k) {
        uint64_t acc = p.atom_off[k];
        for (int t = 0; t < TS; ++t) {
            start[(size_t)t * NBK + k] = acc;
            acc += cnt[(size_t)t * NBK + k];
        }
        p.atom_off[k + 1] = acc;
    }
    const uint64_t A = p.atom_off[NBK];
    if (A == 0) return "block schedule: a part without edges";
    w.av.resize(A);
    w.ac.resize(A);
    w.aw.resize(A);
    par_for(TS, TS, [&](int t) {
        uint64_t* pos = start.data() + (size_t)t * NBK;
        each_atom(vs[t], vs[t + 1], [&](int64_t v, int64_t x, double m) {
            if (m <= 0) return;
            const uint64_t i = pos[bucket_of(x)]++;
            w.av[i] = (int32_t)v;
            w.ac[i] = id_of(x);
            w.aw[i] = m;
        });
    });
    return "";
}

// LINE-2: this part's sample mass per cell, from its atoms
void atom_masses(Work& w, BlockPlan& p) {
    const int nb = w.nb, NBK = w.NBK;
    const int64_t V = w.V, H = w.H;
    std::vector<double> m((size_t)NBK, 0.0);
    for (int k = 0; k < NBK; ++k)
        for (uint64_t i = p.atom_off[k]; i < p.atom_off[k + 1]; ++i) m[k] += w.aw[i];
    if (H > 0) {
        w.mH = m[nb];
        p.hub_off = p.atom_off[nb];
        p.nhub = p.atom_off[nb + 1] - p.atom_off[nb];
        w.hubw.assign((size_t)H, 0.0);
        for (uint64_t i = p.hub_off; i < p.hub_off + p.nhub; ++i) w.hubw[w.ac[i] - V] += w.aw[i];
    }
    // a cell's mass: its block's atoms plus 1/nb of the part's hub atoms
    double tot = 0.0;
    for (int k = 0; k < nb; ++k) {
        p.mass[k] = m[k] + w.mH / nb;
        p.hub_p[k] = p.mass[k] > 0 ? (w.mH / nb) / p.mass[k] : 0.0;
        tot += p.mass[k];
    }
    for (double& x : p.mass) x /= tot;
}

// a walk cell's C-row law: hot_maps.cpp build_hot_maps' scaled law (hot_pc);
// the hub slots at their global rate
void walk_cell_law(const Work& w, BlockPlan& p, int k, double wmax) {
    const std::vector<double>&pn = w.law.pn, &pc = w.law.pc;
    const int64_t lo = p.cb[k], n = p.cb[k + 1] - lo, H = w.H;
    const int K = w.a.K, nb = w.nb;
    const bool hyb = w.a.hybrid;
    auto& pcx = p.pcb[k];
    double mx = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        pcx[i] = w.is_hub(lo + i) ? 0.0 : (pc[lo + i] + K * pn[lo + i]) * nb;
        p.hcb[k][i] = hyb && !w.is_hub(lo + i) ? w.a.hot_c[lo + i] : 0;
        mx = std::max(mx, pcx[i]);
    }
    for (int64_t j = 0; j < H; ++j) {
        pcx[n + j] = p.hub_rate[j];
        p.hcb[k][n + j] = hyb && (double)w.a.M * p.hub_rate[j] > w.a.tau;
        mx = std::max(mx, pcx[n + j]);
    }
    p.pmax_w[k] = wmax;
    p.pmax_c[k] = mx;
}

// a LINE-2 cell's laws, exact from its atoms -- W row v: its atoms' share of
// the cell's mass; C row x: its atoms' share plus K times its share of the
// block's negative law -- so a row is atomic iff M * p > tau in the launch
// that trains it (a scaled global law misses the sources whose contexts crowd
// one block: up to nb times hotter in that cell)
void line2_cell_law(Work& w, BlockPlan& p, int k) {
    const std::vector<double>& pn = w.law.pn;
    const int64_t lo = p.cb[k], n = p.cb[k + 1] - lo, H = w.H, wlo = w.wlo;
    const int K = w.a.K, nb = w.nb;
    const double M = (double)w.a.M, tau = w.a.tau;
    auto& pcx = p.pcb[k];
    std::vector<double> pw((size_t)(w.whi - wlo), 0.0);
    double mraw = 0.0;   // the cell's raw atom mass (its block's, plus 1/nb of the hub atoms')
    for (uint64_t i = p.atom_off[k]; i < p.atom_off[k + 1]; ++i) {
        pw[w.av[i] - wlo] += w.aw[i];
        pcx[w.ac[i] - lo] += w.aw[i];
        mraw += w.aw[i];
    }
    for (uint64_t i = p.hub_off; i < p.hub_off + p.nhub; ++i) pw[w.av[i] - wlo] += w.aw[i] / nb;
    for (int64_t j = 0; j < H; ++j) pcx[n + j] = w.hubw[j] / nb;
    mraw += w.mH / nb;
    w.hwb[k].assign(pw.size(), 0);
    double mw = 0.0, mc = 0.0;
    for (size_t i = 0; i < pw.size(); ++i) {
        w.hwb[k][i] = mraw > 0 && M * pw[i] / mraw > tau;
        if (mraw > 0) mw = std::max(mw, pw[i] / mraw);
    }
    const double pnb = w.nraw[k];
    for (int64_t i = 0; i < n + H; ++i) {
        const double pneg = i < n ? (w.is_hub(lo + i) ? 0.0 : pn[lo + i]) : pn[p.hubs[i - n]] / nb;
        pcx[i] = (mraw > 0 ? pcx[i] / mraw : 0.0) + (pnb > 0 ? K * pneg / pnb : 0.0);
        p.hcb[k][i] = M * pcx[i] > tau;
        mc = std::max(mc, pcx[i]);
    }
    p.pmax_w[k] = mw;
    p.pmax_c[k] = mc;
}

// per block: the C-row law of its cell (over [cb[k], cb[k+1]) then the H
// hub slots) and the flags of its C rows and (LINE-2) of this part's W rows;
// the hottest row of each cell (its launch's concurrency cap, cell_grid):
// walks the scaled global law, LINE-2 the cell's exact one
void cell_laws_and_tags(Work& w, BlockPlan& p) {
    const int nb = w.nb;
    const int64_t H = w.H;
    const bool hyb = w.a.hybrid, walk = w.a.walk;
    p.pcb.assign((size_t)nb, {});
    p.hcb.assign((size_t)nb, {});
    w.hwb.assign((size_t)nb, {});
    p.pmax_w.assign((size_t)nb, 0.0);
    p.pmax_c.assign((size_t)nb, 0.0);
    double wmax = 0.0;
    for (int64_t v = w.wlo; v < w.whi; ++v) wmax = std::max(wmax, w.law.ps[v] * w.a.nparts);
    par_for(nb, w.T, [&](int k) {
        const int64_t n = p.cb[k + 1] - p.cb[k];
        p.pcb[k].assign((size_t)(n + H), 0.0);
        p.hcb[k].assign((size_t)(n + H), 0);
        if (walk) walk_cell_law(w, p, k, wmax);
        else line2_cell_law(w, p, k);
    });
    // one tag per hub slot and per W row of the shared hub atoms (a row's
    // tag must not depend on the cell that draws it): hot in any cell
    w.hubhot.assign((size_t)H, 0);
    if (H > 0 && hyb && walk) {
        const int64_t n0 = p.cb[1] - p.cb[0];
        for (int64_t j = 0; j < H; ++j) w.hubhot[j] = p.hcb[0][n0 + j];
    } else if (H > 0 && hyb) {
        w.hwh.assign((size_t)(w.whi - w.wlo), 0);
        for (int k = 0; k < nb; ++k) {
            const int64_t n = p.cb[k + 1] - p.cb[k];
            for (int64_t j = 0; j < H; ++j) w.hubhot[j] |= p.hcb[k][n + j];
            for (size_t i = 0; i < w.hwh.size(); ++i) w.hwh[i] |= w.hwb[k][i];
        }
        for (int k = 0; k < nb; ++k) {
            const int64_t n = p.cb[k + 1] - p.cb[k];
            for (int64_t j = 0; j < H; ++j) p.hcb[k][n + j] = w.hubhot[j];
        }
    }
}

// LINE-2: one alias table per block over its atoms and one over the part's
// hub atoms, tagged per cell (the hub atoms with their any-cell tags).  The
// atoms' scratch ends here.
void atom_tables(Work& w, BlockPlan& p) {
    const int64_t wlo = w.wlo;
    const bool hyb = w.a.hybrid;
    p.atoms.resize((size_t)p.atom_off[w.NBK] * 8);
    uint32_t* at = p.atoms.data();
    auto table = [&](int k, uint64_t a0, uint64_t n, bool hubs) {
        if (n == 0) return;
        std::vector<double> prob(n);
        std::vector<int64_t> alias(n);
        std::vector<AliasEntry> e(n);
        alias_go(w.aw.data() + a0, (int64_t)n, 1.0, prob.data(), alias.data());
        alias_encode(prob.data(), alias.data(), (int64_t)n, nullptr, e.data());
        auto tw = [&](int32_t v) -> uint32_t { return hubs ? (hyb ? w.hwh[v - wlo] : 0u) : w.hw(k, v); };
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t s = a0 + i, a = a0 + (uint64_t)e[i].alias;
            const uint32_t words[8] = {e[i].thresh,
                                       (uint32_t)w.av[s] | (tw(w.av[s]) << 30),
                                       (uint32_t)w.ac[s] | (w.hc(p, k, w.ac[s]) << 30),
                                       0u,
                                       (uint32_t)w.av[a] | (tw(w.av[a]) << 30),
                                       (uint32_t)w.ac[a] | (w.hc(p, k, w.ac[a]) << 30),
                                       0u,
                                       0u};
            std::copy(words, words + 8, at + 8 * s);
        }
    };
    par_for(w.nb, w.T, [&](int k) { table(k, p.atom_off[k], p.atom_off[k + 1] - p.atom_off[k], false); });
    if (w.H > 0) table(0, p.hub_off, p.nhub, true);
    std::vector<int32_t>().swap(w.av);
    std::vector<int32_t>().swap(w.ac);
    std::vector<double>().swap(w.aw);
    std::vector<std::vector<uint8_t>>().swap(w.hwb);
}

// negative tables: block k's law over its non-hub rows and 1/nb of every
// hub's (Go alias rule, power 1: any exact encoding of the law), ids
// absolute (hub slots V + j); entries of the rows in place, of the slots
// at [k * H, (k + 1) * H)
void negative_tables(Work& w, BlockPlan& p) {
    const std::vector<double>& pn = w.law.pn;
    const int64_t V = w.V, H = w.H;
    const int nb = w.nb;
    p.ntab.resize((size_t)V);
    p.hub_ntab.resize((size_t)nb * (size_t)H);
    par_for(nb, w.T, [&](int k) {
        const int64_t lo = p.cb[k], n = p.cb[k + 1] - lo, nn = n + H;
        std::vector<double> wt((size_t)nn), prob((size_t)nn);
        std::vector<int64_t> alias((size_t)nn);
        std::vector<int32_t> self((size_t)nn);
        auto id = [&](int64_t i) { return (int32_t)(i < n ? lo + i : V + (i - n)); };
        for (int64_t i = 0; i < nn; ++i) {
            wt[i] = i < n ? (w.is_hub(lo + i) ? 0.0 : pn[lo + i]) : pn[p.hubs[i - n]] / nb;
            self[i] = id(i);
        }
        alias_go(wt.data(), nn, 1.0, prob.data(), alias.data());
        for (int64_t i = 0; i < nn; ++i) alias[i] = id(alias[i]);
        std::vector<AliasEntry> e((size_t)nn);
        alias_encode(prob.data(), alias.data(), nn, self.data(), e.data());
        for (int64_t i = 0; i < nn; ++i) {
            const uint32_t al = (uint32_t)e[i].alias;
            e[i].alias = (int32_t)(al | (w.hc(p, k, al) << 30) | (w.hc(p, k, self[i]) << 31));
            if (i < n) p.ntab[lo + i] = e[i];
            else p.hub_ntab[(size_t)k * H + (i - n)] = e[i];
        }
    });
    if (H > 0 && w.a.walk) {   // the pair kernels' hub lookup: slot j | hot tag << 30
        p.hub_of.assign((size_t)V, -1);
        for (int64_t j = 0; j < H; ++j) p.hub_of[p.hubs[j]] = (int32_t)(j | ((int64_t)w.hubhot[j] << 30));
    }
}

}  // namespace

std::string build_block_plan(const HostGraph& g, const DrawLaws& laws, const BlockPlanArgs& a, BlockPlan& p) {
    Work w(g, laws, a);
    std::string err;
    p = BlockPlan{};
    pick_hubs(w, p);
    if (!(err = cut_parts_and_blocks(w, p)).empty()) return err;
    negative_and_part_mass(w, p);
    p.mass.assign((size_t)w.nb, 0.0);
    p.hub_p.assign((size_t)w.nb, 0.0);
    p.atom_off.assign((size_t)w.NBK + 1, 0);
    if (!a.walk) {
        if (!(err = bucket_atoms(w, p)).empty()) return err;
        atom_masses(w, p);
    }
    cell_laws_and_tags(w, p);
    // the atom tables first: they end the atoms' scratch (16 B per atom, C4
    // at 2 parts: ~200 M atoms) before the negative tables are made
    if (!a.walk) atom_tables(w, p);
    negative_tables(w, p);
    return "";
}

}  // namespace smore
