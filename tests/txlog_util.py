"""Test-side helpers of the dated transmission log (reina_model_amd/txlog.py): synthetic states with log words of every code
combination, a plain per-agent walker that counts every field of a report directly, the per-day facts of a simulated run, and
writing a synthetic state into an engine.

A synthetic state is NOT one a simulation could reach; it only ever goes through a report.  Never step a day on one."""
import bisect
from datetime import date

import numpy as np

import tx_util
from tx_util import assert_words  # noqa: F401  (txlog_util.assert_words: the one of every report util)
from reina_model_amd import engine as eng
from reina_model_amd import reports
from reina_model_amd import txlog as txl

SIZES = (1, 511, 512, 513, 3 * 512 + 7)
N_DAYS = 300                      # the synthetic reports' n_days: some of their known days lie beyond
ACTIVE = 0x8000
CODES = (txl.NONE, txl.BEFORE, None)   # None: a known day


def random_log(n, seed=0, top=400):
    """log words of every code combination: each half NONE, BEFORE or a day in [0, top), a third each"""
    rng = np.random.default_rng([n, seed, 77])

    def half():
        kind = rng.integers(0, 3, size=n)
        day = rng.integers(0, top, size=n)
        return np.where(kind == 0, txl.NONE, np.where(kind == 1, txl.BEFORE, day)).astype(np.uint32)

    return half() | half() << 16


def forest_state(n, pattern, seed=0):
    """(hot, infector, n_infected, log) of a tx_util forest with random log words"""
    hot, inf, cnt = tx_util.forest(n, pattern, seed=seed)
    return hot, inf, cnt, random_log(n, seed)


def combos_state():
    """(hot, infector, n_infected, log): one link i <- s for every combination of codes (NONE / BEFORE / known, infection and
    onset, infector and agent: 81 pairs), and links at, and one beyond, both ends of every interval histogram; a negative
    generation interval among them"""
    pairs = []   # ((t_s, o_s), (t_i, o_i))
    for ts in CODES:
        for os_ in CODES:
            for ti in CODES:
                for oi in CODES:
                    k = lambda c, d: d if c is None else c
                    pairs.append(((k(ts, 100), k(os_, 104)), (k(ti, 103), k(oi, 109))))
    for gen in (-3, 0, 1, 63, 64, 200):
        pairs.append(((120, txl.NONE), (120 + gen, txl.NONE)))
    for ser in (-40, -33, -32, -31, 0, 94, 95, 96, 150):
        pairs.append(((txl.BEFORE, 150), (txl.BEFORE, 150 + ser)))
    for tost in (-30, -25, -24, -23, 0, 38, 39, 40, 90):
        pairs.append(((txl.NONE, 150), (150 + tost, txl.NONE)))
    for inc in (-2, 0, 62, 63, 64, 120):
        pairs.append(((10, 12), (40, 40 + inc)))
    pairs.append(((N_DAYS - 1, N_DAYS), (N_DAYS, N_DAYS + 5)))   # known days at and beyond n_days
    n = 2 * len(pairs) + 5
    rng = np.random.default_rng(5)
    hot = np.zeros(n, dtype=np.uint32)
    inf = np.full(n, -1, dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    log = np.full(n, txl.NONE << 16 | txl.NONE, dtype=np.uint32)
    order = rng.permutation(n)
    who = order[:2 * len(pairs)]
    hot[who] = tx_util.hot_word(rng, len(who))
    for k, ((ts, os_), (ti, oi)) in enumerate(pairs):
        s, i = int(who[2 * k]), int(who[2 * k + 1])
        inf[i] = s
        cnt[s] = 1 + k % 5
        log[s] = os_ << 16 | ts
        log[i] = oi << 16 | ti
    # a bad link and a susceptible agent whose log word says otherwise (ignored: the hot word decides who is infected)
    inf[who[1]] = n + 3
    log[order[-1]] = 7 << 16 | 5
    return hot, inf, cnt, log


def assert_same_links(tree, log):
    """a TransmissionReport and a LogReport of ONE state classify its agents alike: infected, roots, links, bad links, and the
    links of every variant (the age matrix summed over its groups == the link phases summed)"""
    assert tree.n_infected_agents == log.infected
    assert tree.n_roots == log.infected - log.links - log.bad_links
    assert tree.n_linked == log.links
    assert tree.bad_links == log.bad_links
    got, want = tree.matrix.sum(axis=(1, 2)), log.link_phase.sum(axis=1)
    assert [int(x) for x in got] == [int(x) for x in want]


def walk_report(hot, infector, n_infected, log, age_start, age_group, n_days):
    """Every field of a report, counted agent by agent in plain Python (independent of report_numpy)"""
    n = len(hot)
    hot = [int(x) for x in np.asarray(hot, dtype=np.uint32)]
    src = [int(x) for x in np.asarray(infector, dtype=np.int32)]
    cnt = [int(x) for x in np.asarray(n_infected, dtype=np.int32).view(np.uint32)]
    log = [int(x) for x in np.asarray(log, dtype=np.uint32)]
    starts = [int(x) for x in age_start]
    nr_ages = len(age_group)
    age = lambda i: min(max(bisect.bisect_right(starts[:nr_ages + 1], i) - 1, 0), nr_ages - 1)
    known = lambda x: x not in (txl.NONE, txl.BEFORE)
    clip = lambda x, bins: min(max(x, 0), bins - 1)
    incub = np.zeros((4, 64), dtype=np.uint64)
    gen = np.zeros((4, 64), dtype=np.uint64)
    ser = np.zeros((4, 128), dtype=np.uint64)
    tost = np.zeros((4, 64), dtype=np.uint64)
    phase = np.zeros((4, 4), dtype=np.uint64)
    incidence = np.zeros((n_days, 4, 16), dtype=np.uint64)
    onsets = np.zeros((n_days, 4), dtype=np.uint64)
    cohort = np.zeros((n_days, 4, 3), dtype=np.uint64)
    sc = {name: 0 for name in txl.SCALAR_NAMES}
    first, last = None, None
    for i in range(n):
        h = hot[i]
        if h & 7 == 0:
            continue
        v = (h >> 8) & 3
        t, o = log[i] & 0xFFFF, log[i] >> 16
        sc['infected'] += 1
        if t == txl.BEFORE:
            sc['before'] += 1
        if known(t):
            sc['dated'] += 1
            first = t if first is None else min(first, t)
            last = t if last is None else max(last, t)
            if t < n_days:
                incidence[t, v, age_group[age(i)]] += 1
                cohort[t, v, 0] += 1
                cohort[t, v, 1] += cnt[i]
                if h & 7 >= 5:
                    cohort[t, v, 2] += 1
            else:
                sc['out_of_range'] += 1
        if known(o):
            sc['with_onset'] += 1
            if o < n_days:
                onsets[o, v] += 1
            else:
                sc['out_of_range'] += 1
        if known(t) and known(o):
            incub[v, clip(o - t, 64)] += 1
        s = src[i]
        if s == -1:
            continue
        if not (0 <= s < n and s != i and hot[s] & 7 != 0):
            sc['bad_links'] += 1
            continue
        sc['links'] += 1
        ts, os_ = log[s] & 0xFFFF, log[s] >> 16
        if known(t) and known(ts):
            sc['links_dated'] += 1
            if t <= ts:
                sc['generation_nonpositive'] += 1
            gen[v, clip(t - ts, 64)] += 1
        if known(o) and known(os_):
            ser[v, clip(o - os_ + 32, 128)] += 1
        if known(t) and known(os_):
            tost[v, clip(t - os_ + 24, 64)] += 1
            phase[v, 0 if t < os_ else 1] += 1
        elif known(t) and os_ == txl.NONE:
            phase[v, 2] += 1
        else:
            phase[v, 3] += 1
    sc['first_day'] = (1 << 64) - 1 if first is None else first
    sc['last_day'] = 0 if last is None else last
    w = np.concatenate([incub.ravel(), gen.ravel(), ser.ravel(), tost.ravel(), phase.ravel(),
                        np.array([sc[name] for name in txl.SCALAR_NAMES] + [0] * (txl.S_NR - len(txl.SCALAR_NAMES)), dtype=np.uint64),
                        incidence.ravel(), onsets.ravel(), cohort.ravel()])
    assert len(w) == txl.report_words(n_days)
    return w


def record_by_hot(log, hot, day):
    """what k_txlog_day's hot-word form stores on a day that follows a recorded day: an ACTIVE agent in INCUBATION with the day
    in bits 24-31 gets the whole word NONE << 16 | day, one in ILLNESS with day + 1 there the day in its upper half; nothing else
    is touched"""
    hot = np.asarray(hot, dtype=np.uint32)
    out = np.array(log, dtype=np.uint32)
    act, st, hi = (hot & ACTIVE) != 0, hot & 7, hot >> 24
    new = act & (st == 1) & (hi == (day & 0xFF))
    ons = act & (st == 2) & (hi == ((day + 1) & 0xFF))
    out[new] = txl.NONE << 16 | day
    out[ons] = (out[ons] & 0xFFFF) | np.uint32(day << 16)
    return out


class DayFacts:
    """run_host_driven's on_day handle: asserts, after every day, what k_txlog_day may rely on, and keeps the day's numbers"""

    def __init__(self, check_planes=None):
        self.dated, self.onsets = {}, {}
        self.first = True
        self.check_planes = check_planes   # (GPU engines: a callable that compares the ACTIVE bit plane with the hot words)

    def __call__(self, day, hot, before, after):
        new = ((before & 0xFFFF) == txl.NONE) & ((after & 0xFFFF) != txl.NONE)
        ons = ((before >> 16) == txl.NONE) & ((after >> 16) != txl.NONE)
        w = hot[new]
        assert ((w & ACTIVE) != 0).all(), 'day %d: a newly infected agent is not ACTIVE' % day
        assert ((w & 7) == 1).all(), 'day %d: a newly infected agent is not INCUBATION' % day
        assert ((w >> 24) == (day & 0xFF)).all(), 'day %d: bits 24-31 of a newly infected agent' % day
        w = hot[ons]
        assert ((w & ACTIVE) != 0).all(), 'day %d: an onset on an agent that is not ACTIVE' % day
        assert ((w & 7) == 2).all(), 'day %d: an onset first seen in a state other than ILLNESS' % day
        assert ((w >> 24) == ((day + 1) & 0xFF)).all(), 'day %d: bits 24-31 of an onset' % day
        if not self.first:
            assert np.array_equal(record_by_hot(before, hot, day), after), 'day %d: the hot-word form differs from the definition' % day
        self.first = False
        self.dated[day] = int(new.sum())
        self.onsets[day] = int(ons.sum())
        if self.check_planes is not None:
            self.check_planes(day, hot)


def pre_init_imports(ctx):
    """{day: summed amount} of the Context's import-infections interventions (the pre_init batches new_infections leaves out)"""
    d0 = date.fromisoformat(str(ctx.start_date))
    out = {}
    for iv in ctx.interventions:
        if iv.type == 'import-infections':
            k = (ctx._iv_date(iv) - d0).days
            out[k] = out.get(k, 0) + int(iv.values['amount'])
    return out


def new_infections(hist, final_counters):
    """new_infections totals as read AFTER each day: history row d + 1, the final counter block for the last day"""
    rows = np.concatenate([np.asarray(hist)[1:], np.asarray(final_counters)[None, :]])
    ci = eng.C_NAMES.index('new_infections')
    return rows[:, ci * eng.MAX_AGES:(ci + 1) * eng.MAX_AGES].astype(np.int64).sum(axis=1)


def host_state(ctx):
    """(hot, infector, n_infected) of a Context's engine, host copies (reports.host_state, which hands out views of a
    host-memory engine's buffers)"""
    hot, infector, n_infected, _ = reports.host_state(ctx.engine)
    return hot.copy(), infector.view(np.int32).copy(), n_infected.view(np.int32).copy()


def spec_report(ctx, log_words, n_days=None, groups=None):
    """report_numpy of a Context's state with the given log words"""
    hot, inf, cnt = host_state(ctx)
    table = ctx._tx_groups(groups)[0]
    return txl.report_numpy(hot, inf, cnt, log_words, ctx.age_start, table, max(ctx.day, 1) if n_days is None else n_days)
