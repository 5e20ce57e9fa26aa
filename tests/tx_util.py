"""Test-side helpers for transmission reports: synthetic forests (hot words + infector links + infection counts) of any size, a
plain per-agent walker that counts every field of a report directly, and writing a forest into an engine.

A synthetic forest is NOT a state a simulation could reach (its n_infected need not match the links, its hot words carry random
countdown bits); it only ever goes through a report, which reads hot, infector and n_infected.  Never step a day on one."""
import bisect

import numpy as np

from reina_model_amd import engine as eng
from reina_model_amd import transmission as tx

PATTERNS = ('empty', 'roots', 'chain', 'star', 'giant', 'random', 'bad_links')
NR_AGES = 101


def age_start_of(n):
    """age_start[MAX_AGES + 1] of snap_util.population(n) (all in age 40 below 101 agents, spread evenly otherwise)"""
    ages = np.zeros(NR_AGES, dtype=np.int64)
    if n < NR_AGES:
        ages[40] = n
    else:
        ages[:] = n // NR_AGES
        ages[:n % NR_AGES] += 1
    s = np.zeros(eng.MAX_AGES + 1, dtype=np.int64)
    s[1:NR_AGES + 1] = np.cumsum(ages)
    s[NR_AGES + 1:] = n
    return s


def groups(kind='default'):
    """a per-age group table: 'default' 10-year bins and 80+, 'fine' 16 groups of 7 years"""
    a = np.arange(NR_AGES)
    return np.minimum(a // 10, 8) if kind == 'default' else np.minimum(a // 7, 15)


def hot_word(rng, n, states=(1, 2, 3, 4, 5, 6)):
    """random infected hot words: every variant, severity 0..4, the given states, detected / included bits, random high bits"""
    st = rng.choice(np.asarray(states, dtype=np.uint32), size=n)
    sev = rng.integers(0, 5, size=n, dtype=np.uint32)
    det = rng.integers(0, 2, size=n, dtype=np.uint32)
    var = rng.integers(0, 4, size=n, dtype=np.uint32)
    inc = rng.integers(0, 2, size=n, dtype=np.uint32)
    high = rng.integers(0, 1 << 21, size=n, dtype=np.uint32)
    return (st | sev << 3 | det << 6 | var << 8 | inc << 10 | high << 11).astype(np.uint32)


def forest(n, pattern, seed=0, size=None):
    """(hot uint32[n], infector int32[n], n_infected int32[n]) of a named pattern; `size`: the chain's / star's / giant
    tree's number of agents (default: all n)"""
    rng = np.random.default_rng([n, PATTERNS.index(pattern), seed])
    hot = np.zeros(n, dtype=np.uint32)
    inf = np.full(n, -1, dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    m = n if size is None else min(size, n)
    if pattern == 'empty':
        return hot, inf, cnt
    if pattern == 'roots':
        hot[:] = hot_word(rng, n)
        cnt[:] = rng.integers(0, 70, size=n)
        return hot, inf, cnt
    if pattern in ('chain', 'star', 'giant'):
        who = rng.permutation(n)[:m]        # the tree's agents, in the order they were infected
        hot[who] = hot_word(rng, m)
        if pattern == 'chain':
            inf[who[1:]] = who[:-1]
        elif pattern == 'star':
            inf[who[1:]] = who[0]
        else:
            inf[who[1:]] = who[(rng.random(m - 1) * np.arange(1, m)).astype(np.int64)]
        np.add.at(cnt, inf[who[1:]], 1)
        return hot, inf, cnt
    # random forests: a share of the agents infected, ~1/8 of them roots, the others linked to an earlier infected agent
    infected = rng.permutation(n)[:int(0.6 * n) + (1 if n else 0)]
    k = len(infected)
    hot[infected] = hot_word(rng, k)
    is_root = rng.random(k) < 0.125
    if k:
        is_root[0] = True
    pick = (rng.random(k) * np.arange(k)).astype(np.int64)
    inf[infected[~is_root]] = infected[pick[~is_root]]
    cnt[infected] = rng.integers(0, 90, size=k)
    if pattern == 'bad_links' and k >= 4:
        sus = np.flatnonzero(hot == 0)
        plant = rng.choice(k, size=max(4, k // 20), replace=False)
        for j, a in enumerate(infected[plant]):
            kind = j % 4
            inf[a] = (n + int(rng.integers(0, 1000)), a, -7, sus[j % len(sus)] if len(sus) else a)[kind]
    return hot, inf, cnt


def walk_report(hot, infector, n_infected, age_start, age_group, max_depth):
    """Every field of a report, counted agent by agent with dicts and plain Python (independent of report_numpy)"""
    n = len(hot)
    hot = [int(x) for x in np.asarray(hot, dtype=np.uint32)]
    src = [int(x) for x in np.asarray(infector, dtype=np.int32)]
    cnt = [int(x) for x in np.asarray(n_infected, dtype=np.int32).view(np.uint32)]
    starts = [int(x) for x in age_start]
    nr_ages = len(age_group)
    age = lambda i: min(max(bisect.bisect_right(starts[:nr_ages + 1], i) - 1, 0), nr_ages - 1)
    rounds = tx.rounds_for(max_depth)
    reach = (1 << rounds) - 1      # after r rounds every agent within 2^r - 1 links of its root has found it
    w = np.zeros(tx.REPORT_WORDS, dtype=np.uint64)
    off = np.zeros((4, 5, 3, 2, 64), dtype=np.uint64)
    sums = np.zeros((4, 3), dtype=np.uint64)
    sq = np.zeros((4, 3), dtype=np.uint64)
    mat = np.zeros((4, 16, 16), dtype=np.uint64)
    gens = np.zeros((4, 256), dtype=np.uint64)
    sc = dict(n_infected_agents=0, n_roots=0, n_linked=0, bad_links=0, unconverged=0, max_generation=0)
    link = {}
    for i in range(n):
        h = hot[i]
        if h & 7 == 0:
            continue
        st, v, sev = h & 7, (h >> 8) & 3, min((h >> 3) & 7, 4)
        o = 0 if st <= 4 else (1 if h & 0x400 else 2)
        d = 1 if h & 0x40 else 0
        off[v, sev, o, d, min(cnt[i], 63)] += 1
        sums[v, o] += cnt[i]
        sq[v, o] += cnt[i] * cnt[i]
        sc['n_infected_agents'] += 1
        s = src[i]
        if s == -1:
            sc['n_roots'] += 1
            link[i] = None
        elif 0 <= s < n and s != i and hot[s] & 7 != 0:
            sc['n_linked'] += 1
            link[i] = s
            mat[v, age_group[age(s)], age_group[age(i)]] += 1
        else:
            sc['bad_links'] += 1
            link[i] = None
    found = {}   # agent -> (root, generation)

    def root_of(i):
        path = []
        while i not in found and link[i] is not None and len(path) <= n:
            path.append(i)
            i = link[i]
        r, g = found[i] if i in found else ((i, 0) if link[i] is None else (None, None))
        for a in reversed(path):
            g = None if g is None else g + 1
            found[a] = (r, g)
        if not path:
            found[i] = (r, g)
        return found[path[0]] if path else found[i]

    size = {}
    for i in link:
        r, g = root_of(i)
        if r is None or g > reach:
            sc['unconverged'] += 1
            continue
        gens[(hot[i] >> 8) & 3, min(g, 255)] += 1
        sc['max_generation'] = max(sc['max_generation'], g)
        size[r] = size.get(r, 0) + 1
    cl = np.zeros(33, dtype=np.uint64)
    ca = np.zeros(33, dtype=np.uint64)
    largest, lroot = 0, None
    for r in sorted(size):
        b = size[r].bit_length() - 1
        cl[b] += 1
        ca[b] += size[r]
        if size[r] > largest:
            largest, lroot = size[r], r
    w[tx.OFFSPRING:tx.OFFSPRING_SUM] = off.ravel()
    w[tx.OFFSPRING_SUM:tx.OFFSPRING_SUMSQ] = sums.ravel()
    w[tx.OFFSPRING_SUMSQ:tx.MATRIX] = sq.ravel()
    w[tx.MATRIX:tx.GENERATION] = mat.ravel()
    w[tx.GENERATION:tx.CLUSTERS] = gens.ravel()
    w[tx.CLUSTERS:tx.CLUSTER_AGENTS] = cl
    w[tx.CLUSTER_AGENTS:tx.SCALARS] = ca
    sc.update(sum_n_infected=int(sums.sum()), largest_cluster=largest, rounds=rounds,
              largest_root=(1 << 64) - 1 if lroot is None else lroot,
              largest_key=0 if lroot is None else largest << 32 | (~lroot & 0xFFFFFFFF))
    for k, name in enumerate(tx.SCALAR_NAMES):
        w[tx.SCALARS + k] = sc[name]
    return w


def assert_words(got, want):
    """two reports' words are the same; the first differing ones otherwise (every report util's assert_words)"""
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not len(bad), [(int(k), int(got[k]), int(want[k])) for k in bad[:8]]


def put_forest(ctx, hot, infector, n_infected, day=None):
    """write a forest into a Context's engine (numpy or torch tensors); `day`: the counter block's REINA_S_DAY word"""
    t = ctx.engine.tensors
    n = ctx.engine.config.n_agents
    cold = np.zeros((n, eng.COLD_WORDS), dtype=np.int32)
    cold[:, 2] = infector
    cold[:, 3] = n_infected
    if hasattr(t['hot'], 'copy_'):
        import torch
        t['hot'].copy_(torch.from_numpy(np.asarray(hot, dtype=np.uint32).view(np.int32)))
        t['cold'].view(n, eng.COLD_WORDS)[:, 2:4].copy_(torch.from_numpy(cold[:, 2:4].copy()))
        if day is not None:
            t['counters'][eng.C_NR * eng.MAX_AGES + eng.S_DAY] = int(day)
    else:
        np.asarray(t['hot']).view(np.uint32)[:] = hot
        np.asarray(t['cold']).reshape(n, eng.COLD_WORDS)[:, 2:4] = cold[:, 2:4]
        if day is not None:
            np.asarray(t['counters'])[eng.C_NR * eng.MAX_AGES + eng.S_DAY] = int(day)
