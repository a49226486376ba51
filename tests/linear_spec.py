"""The linearised fp64 reference of a batch of update records (test
infrastructure: the checker of the lossless parallel scatter modes, never the
product).

For records s = 0 .. n-1 and initial tables T0

    L = T0 + sum_s D_s(T0),

D_s(T0) being sample s's complete update evaluated in fp64 on the INITIAL
tables (fastSigmoid table, the in-sample in-place semantics of repeated ids).
L does not depend on the order of the samples.  A lossless parallel launch
gives T0 + sum_s D_s(T_read_s) plus fp32 rounding: with a small step the
difference from L is second order in alpha, while a dropped, doubled or
misrouted sample is first order.

The rules restate oracle/smore_oracle.c's fp64 functions row by row (a row op
here is the oracle's element loop: every element op touches one element of
each row, so the aliasing of repeated ids behaves the same):
  cpp     UpdatePair (LINE-2; LINE-1 with the contexts in W itself; the pair
          call), Opt_SGD for MF, a block cell's alpha * neg_scale on negatives
  bpr     UpdateBPRPair, 5 rounds, one table
  go      Go UpdatePair: negatives equal to the context skipped, the
          context's gradient deferred
  gobpr   Go UpdateBPRPair: users W, items C, one negative, lambda
A record is {v, c, n_1 .. n_K}; c < 0 is a skipped sample (no update).
"""
import numpy as np

from oracle import oracle as orc

_SIG = None


def sig(x):
    """fastSigmoid (src/proNet.cpp:52-71) through the oracle's table."""
    global _SIG
    if _SIG is None:
        _SIG = orc.sigmoid_table()
    if x < -8.0:
        return 0.0
    if x > 8.0:
        return 1.0
    return float(_SIG[int((x + 8.0) * 1000 / 8.0 / 2)])


# ---------------------------------------------------------------- rules
# row(t, r) returns the mutable row r of table t; the same array for the same
# (t, r), so a repeated id is updated in place as in the reference.
def rule_cpp(row, rec, alpha, shared=False, mf=False, reg=0.0, neg_scale=1.0):
    v, c = int(rec[0]), int(rec[1])
    tc = 0 if shared else 1
    wv = row(0, v)
    err = np.zeros_like(wv)
    for k, x in enumerate(rec[1:]):
        wc = row(tc, int(x))
        f = float(wv @ wc)
        if mf:
            g = (1.0 if k == 0 else -1.0) - f
            e = alpha * (g * wc - reg * wv)
            wc += alpha * (g * wv - reg * wc)
            err += e
        else:
            g = ((1.0 if k == 0 else 0.0) - sig(f)) * (alpha if k == 0 else alpha * neg_scale)
            err += g * wc
            wc += g * wv
    wv += err
    return c


def rule_bpr(row, rec, alpha):
    wu, wi = row(0, int(rec[0])), row(0, int(rec[1]))
    verr = np.zeros_like(wu)
    for j in rec[2:7]:
        wj = row(0, int(j))
        x = wi - wj
        g = sig(0.0 - float(wu @ x)) * alpha
        verr += g * x
        cerr = g * wu
        wi -= alpha * 0.0025 * wi
        wj -= alpha * 0.0025 * wj
        wi += cerr
        wj -= cerr
    wu -= alpha * 0.025 * wu
    wu += verr


def rule_go(row, rec, alpha):
    c = int(rec[1])
    wv, cc = row(0, int(rec[0])), row(1, c)
    grad = alpha * (1.0 - sig(float(wv @ cc)))
    vg, cg = grad * cc, grad * wv
    for x in rec[2:]:
        if int(x) == c:
            continue
        cn = row(1, int(x))
        grad = alpha * (0.0 - sig(float(wv @ cn)))
        vg += grad * cn
        cn += grad * wv
    wv += vg
    cc += cg


def rule_gobpr(row, rec, alpha, lam=0.0):
    wu, ci, cj = row(0, int(rec[0])), row(1, int(rec[1])), row(1, int(rec[2]))
    pos, neg = float(wu @ ci), float(wu @ cj)
    gc = alpha * sig(neg - pos)
    vgr, pg, ngr = gc * (ci - cj), gc * wu, -gc * wu
    wu += vgr - lam * alpha * wu
    ci += pg - lam * alpha * ci
    cj += ngr - lam * alpha * cj          # cj is ci when j == i: the updated row


RULES = {"cpp": rule_cpp, "bpr": rule_bpr, "go": rule_go, "gobpr": rule_gobpr}


def live(records):
    """The records that update (c >= 0)."""
    return np.asarray(records)[:, 1] >= 0


# ---------------------------------------------------------------- rates
def rates(kind, begin, n, alpha0, total):
    """fp64 rate of records begin .. begin + n - 1: "line" (LINE counts from 1),
    "mf" (MF / BPR from 0), "go" (the Go schedule), "fixed"."""
    if kind == "fixed":
        return np.full(n, float(alpha0))
    if kind == "go":
        return np.array([orc.lib().orc_alpha_walk(begin + i, alpha0, total) for i in range(n)])
    base = 1 if kind == "line" else 0
    return np.array([orc.alpha_line(begin + i + base, alpha0, total) for i in range(n)])


# ---------------------------------------------------------------- pair negatives
def pair_negatives(g, n, K, seed, unit):
    """The K negatives of caller pair i (orc_update_pairs_f64's slot layout):
    stream 3, unit `unit` + i // 2^20, slots 2K (i mod 2^20) + 2j (index) and
    + 1 (p), through g's encoded negative table (NegativeSample: index first)."""
    out = np.zeros((n, K), np.int32)
    if K == 0:
        return out
    blk = orc.PAIR_BLOCK
    V = int(g.V)
    for b in range(0, n, blk):
        m = min(blk, n - b)
        w = orc.words(seed, 3, unit + b // blk, 2 * K * m).astype(np.uint64).reshape(m, K, 2)
        idx = ((w[:, :, 0] * np.uint64(V)) >> np.uint64(32)).astype(np.int64)
        keep = w[:, :, 1] < g.nthr[idx].astype(np.uint64)
        out[b:b + m] = np.where(keep, idx, g.nalias_enc[idx])
    return out


def pair_records(g, v, c, K, seed, unit):
    v, c = np.asarray(v, np.int32), np.asarray(c, np.int32)
    return np.concatenate([v[:, None], c[:, None], pair_negatives(g, len(v), K, seed, unit)], axis=1)


# ---------------------------------------------------------------- serial and linearised runs
def serial_f64(tables, records, rule, alphas, **kw):
    """The records in order on fp64 tables, in place."""
    fn = RULES[rule]

    def row(t, r):
        return tables[t][r]
    for rec, a in zip(records, alphas):
        if rec[1] >= 0:
            fn(row, rec, float(a), **kw)
    return tables


def sample_delta(T0s, rec, alpha, rule, **kw):
    """{(table, row): fp64 delta} of one record evaluated on the tables T0s."""
    loc = {}

    def row(t, r):
        k = (t, r)
        if k not in loc:
            loc[k] = np.array(T0s[t][r], np.float64)
        return loc[k]
    if rec[1] < 0:
        return {}
    RULES[rule](row, rec, float(alpha), **kw)
    return {k: x - np.asarray(T0s[k[0]][k[1]], np.float64) for k, x in loc.items()}


class Linear:
    """L per table; the per-sample largest row delta (0 for a skipped record);
    per row touch (sample, table, row) the largest element delta."""

    def __init__(self, L, sample_max, touch_sample, touch_table, touch_row, touch_max):
        self.L, self.sample_max = L, sample_max
        self.touch_sample, self.touch_table, self.touch_row, self.touch_max = (touch_sample, touch_table, touch_row,
                                                                               touch_max)

    def touched(self):
        """Sorted row ids touched, per table."""
        return [np.unique(self.touch_row[self.touch_table == t]) for t in range(len(self.L))]


def linear(T0s, records, rule, alphas, **kw):
    L = [np.array(T, np.float64) for T in T0s]
    n = len(records)
    smax = np.zeros(n)
    ts, tt, tr, tm = [], [], [], []
    for s in range(n):
        for (t, r), d in sample_delta(T0s, records[s], alphas[s], rule, **kw).items():
            L[t][r] += d
            m = float(np.abs(d).max())
            smax[s] = max(smax[s], m)
            ts.append(s); tt.append(t); tr.append(r); tm.append(m)
    return Linear(L, smax, np.array(ts, np.int64), np.array(tt, np.int64), np.array(tr, np.int64), np.array(tm))


# ---------------------------------------------------------------- the fp32 side
def padded(T, dim=None):
    """fp32 [V][dpad] copy (dpad a multiple of 4), the oracle's fp32 layout."""
    T = np.asarray(T)
    out = np.zeros((T.shape[0], (T.shape[1] + 3) // 4 * 4), np.float32)
    out[:, :T.shape[1]] = T
    return out


def gap(L, runs):
    """max |S - L| over the tables, the larger over the fp32 runs `runs` (each
    a list of tables, padded or not: the columns of L count)."""
    worst = 0.0
    for S in runs:
        for Lt, St in zip(L, S):
            worst = max(worst, float(np.abs(np.asarray(St, np.float64)[:, :Lt.shape[1]] - Lt).max()))
    return worst


def rule_f32(tables, records, rule, alphas, **kw):
    """The rule over the records in order on fp32 tables, in place: every row
    operation and dot product in numpy fp32, the rate rounded to fp32 (the
    scalars stay Python floats, which leave fp32 arrays fp32).  A legitimate
    fp32 order for the rules whose oracle fp32 function takes no records."""
    fn = RULES[rule]
    assert all(T.dtype == np.float32 for T in tables)

    def row(t, r):
        return tables[t][r]
    for rec, a in zip(records, alphas):
        if rec[1] >= 0:
            fn(row, rec, float(np.float32(a)), **kw)
    return tables


# ---------------------------------------------------------------- the check
def check(got, T0s, L, tol, touched):
    """max |got - L| <= tol on every table, and every row no record touches is
    bit-equal to T0."""
    for t, (G, T0, Lt) in enumerate(zip(got, T0s, L)):
        G = np.asarray(G)
        d = np.abs(G.astype(np.float64) - Lt)
        worst = np.unravel_index(int(np.argmax(d)), d.shape)
        assert d[worst] <= tol, "table %d row %d: |got - L| = %.3g > tol %.3g (%.1f tol; %d rows over tol)" % (
            t, worst[0], d[worst], tol, d[worst] / tol, int((d.max(axis=1) > tol).sum()))
        rest = np.ones(G.shape[0], bool)
        rest[touched[t]] = False
        bad = np.flatnonzero(rest & (G != np.asarray(T0s[t])).any(axis=1))
        assert bad.size == 0, "table %d: %d untouched rows changed (first %d)" % (t, bad.size, bad[0])


def residual(got, L):
    return max(float(np.abs(np.asarray(G, np.float64) - Lt).max()) for G, Lt in zip(got, L))


def preconditions(lin, records, tol, want_repeat=True, shared=False, want_multi=True, sample_factor=8.0,
                  weak_samples=0.0, touch_cols=None):
    """Conditions of the batch under which `check` at `tol` tells a lost,
    doubled or misrouted update from rounding (asserted from the reference):
    every live sample's largest row delta is at least 8 tol, at most 1 % of
    the row touches have a largest element delta under 2 tol, at least 3 rows
    are touched more than once, some sample repeats an id among its context
    rows (or, with one shared table, has its source among them).
    The BPR rules cannot meet the first two as they stand (one sigmoid gates a
    whole sample, a negative row takes a single small step), so their callers
    state a weaker form: sample_factor, weak_samples (the share of live samples
    allowed under sample_factor x tol) and touch_cols (only the touches of
    these record columns' rows count)."""
    records = np.asarray(records)
    lv = live(records)
    assert lv.any()
    weak = float((lin.sample_max[lv] < sample_factor * tol).mean())
    assert weak <= weak_samples, "%.2f %% of the samples move their rows by under %g tol = %.3g (least %.3g)" % (
        100 * weak, sample_factor, sample_factor * tol, lin.sample_max[lv].min())
    counted = np.ones(len(lin.touch_max), bool)
    if touch_cols is not None:
        counted = (records[lin.touch_sample][:, list(touch_cols)] == lin.touch_row[:, None]).any(axis=1)
    small = float((lin.touch_max[counted] < 2 * tol).mean())
    assert small <= 0.01, "%.2f %% of the row touches are under 2 tol" % (100 * small)
    key = lin.touch_table * (int(lin.touch_row.max()) + 1) + lin.touch_row
    if want_multi:
        assert (np.unique(key, return_counts=True)[1] > 1).sum() >= 3, "fewer than 3 rows touched more than once"
    if want_repeat:
        r = np.asarray(records)[lv]
        srt = np.sort(r[:, 1:], axis=1)
        rep = (srt[:, 1:] == srt[:, :-1]).any(axis=1)
        if shared:
            rep |= (r[:, :1] == r[:, 1:]).any(axis=1)
        assert rep.any(), "no sample with a repeated id"
