"""Test-side helpers of the ensemble summaries (reina_model_amd/summary.py): synthetic histories, specs with thresholds at
values that occur, a plain Python walker of the definition."""
import numpy as np

from reina_model_amd import engine as eng
from reina_model_amd import summary as sm

A, C, CW = eng.MAX_AGES, eng.C_NR, eng.COUNTER_WORDS
PATTERNS = ('random', 'equal', 'ties', 'negative', 'extremes', 'wrap')
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def history(K, days, nr_ages, pattern, seed=0):
    """int32[K, days, COUNTER_WORDS] from a fixed seed; the words of ages >= nr_ages hold garbage"""
    rng = np.random.default_rng(1000 * seed + 17 * K + days + PATTERNS.index(pattern))
    shape = (K, days, CW)
    if pattern == 'random':
        h = rng.integers(0, 1_000_000, shape)
    elif pattern == 'equal':          # every member the same rows
        h = np.broadcast_to(rng.integers(0, 1000, (1, days, CW)), shape).copy()
    elif pattern == 'ties':           # three values: ties everywhere
        h = rng.choice(np.array([0, 7, 8]), shape)
    elif pattern == 'negative':
        h = rng.integers(-50_000, 50_000, shape)
    elif pattern == 'extremes':       # INT32_MIN and INT32_MAX in the scalar slots
        h = rng.integers(-3, 3, shape)
        h[:, :, C * A:] = rng.choice(np.array([I32_MIN, I32_MAX, 0, -1, 1]), (K, days, eng.S_NR))
    elif pattern == 'wrap':           # per-age values whose uint32 sum wraps, with either sign left over
        h = rng.integers(2 ** 29, 2 ** 31 - 1, shape)
    else:
        raise ValueError(pattern)
    h = h.astype(np.int64)
    per_age = h[:, :, :C * A].reshape(K, days, C, A)
    per_age[..., nr_ages:] = rng.integers(I32_MIN, I32_MAX, (K, days, C, A - nr_ages))   # garbage behind the ages
    return h.astype(np.int32)


def groups(G, nr_ages, seed=0):
    """SummarySpec age_groups of exactly G groups (labels g0 .. ), the ages spread over them in no order"""
    rng = np.random.default_rng(seed + 31 * G + nr_ages)
    idx = rng.permutation(np.arange(eng.MAX_AGES) % G)
    return dict(labels=['g%d' % k for k in range(G)], age_indices=idx)


def quantile_levels(Q):
    """Q = 1: the median; Q = 16: ranks 0 and K - 1, repeats, no order"""
    if Q == 1:
        return (0.5,)
    return (1.0, 0.0, 0.5, 0.5, 0.05, 0.95, 0.25, 0.75, 0.0, 1.0, 0.33, 0.66, 0.1, 0.9, 0.01, 0.99)[:Q]


def spec_for(h, nr_ages, G, Q, T, seed=0):
    """a SummarySpec of G groups, Q quantiles and T thresholds, each threshold at a value its series takes somewhere"""
    ag = groups(G, nr_ages, seed)
    base = sm.SummarySpec(quantile_levels(Q), ag)
    lay = sm.Layout(base, h.shape[0], h.shape[1], nr_ages)
    ser = sm.series_numpy(h, nr_ages, lay.table, lay.G)
    rng = np.random.default_rng(seed + 5)
    names = [(a, None) for a in eng.C_NAMES] + [(a, g) for a in eng.C_NAMES[:4] for g in lay.labels] + [(s, None) for s in sm.SCALAR_SLOTS]
    thr = []
    for t in range(T):
        attr, g = names[int(rng.integers(len(names)))]
        s = lay.series(attr, g)
        value = int(ser[int(rng.integers(h.shape[0])), int(rng.integers(h.shape[1])), s])
        thr.append((attr, value) if g is None else (attr, g, value))
    return sm.SummarySpec(quantile_levels(Q), ag, thr)


def walk(h, nr_ages, lay):
    """the block's words by plain Python loops over the definition (tiny inputs only)"""
    K, days, G, S = lay.K, lay.days, lay.G, lay.S
    wrap = lambda x: (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31
    ser = [[[0] * S for _ in range(days)] for _ in range(K)]
    for m in range(K):
        for d in range(days):
            row = [int(x) for x in h[m, d]]
            for c in range(C):
                for a in range(nr_ages):
                    x = row[c * A + a]
                    ser[m][d][c * (1 + G)] += x
                    ser[m][d][c * (1 + G) + 1 + int(lay.table[a])] += x
            for s in range(eng.S_NR):
                ser[m][d][C * (1 + G) + s] = row[C * A + s]
            ser[m][d] = [wrap(x) for x in ser[m][d]]
    w = []
    for d in range(days):
        for s in range(S):
            col = sorted(ser[m][d][s] for m in range(K))
            w += [col[int(r)] for r in lay.ranks]
    w += [sum(ser[m][d][s] for m in range(K)) for d in range(days) for s in range(S)]
    for m in range(K):
        for s in range(S):
            best = max(ser[m][d][s] for d in range(days))
            w += [best, min(d for d in range(days) if ser[m][d][s] == best)]
    w += [ser[m][days - 1][s] for m in range(K) for s in range(S)]
    for s, value in lay.thresholds:
        w += [sum(ser[m][d][s] > value for m in range(K)) for d in range(days)]
    for s, value in lay.thresholds:
        for m in range(K):
            above = [d for d in range(days) if ser[m][d][s] > value]
            w.append(above[0] if above else -1)
    return np.array(w, dtype=np.int64)


def assert_words(got, want, lay):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if len(bad):
        names = ('order', 'sum', 'peak', 'final', 'exceed', 'first_exceed')
        k = int(bad[0])
        table = names[int(np.searchsorted(lay.offsets, k, side='right')) - 1]
        raise AssertionError('%d of %d words differ; the first is word %d (%s + %d): %d, expected %d'
                             % (len(bad), len(got), k, table, k - lay.offsets[names.index(table)], got[k], want[k]))
