"""Test-side helpers of the detection report (reina_model_amd/detection.py): synthetic states with links, log words and course
records of every combination, a plain per-agent and per-link walker that counts every field of a report directly, writing a
synthetic state into an engine, and the specification on a Context's read-back state.

A synthetic state is NOT one a simulation could reach; it only ever goes through a report.  Never step a day on one."""
import bisect

import numpy as np

import course_util
import tx_util
import txlog_util
from tx_util import assert_words  # noqa: F401  (detection_util.assert_words: the one of every report util)
from reina_model_amd import course as crs
from reina_model_amd import detection as det
from reina_model_amd import reports
from reina_model_amd import txlog as txl

N_DAYS = txlog_util.N_DAYS         # the synthetic reports' n_days: some of their known days lie beyond
DETECTED = 0x40
NO, BF = txl.NONE, txl.BEFORE


def forest_state(n, seed=0, pattern='bad_links'):
    """(hot, infector, n_infected, log, rec): a random tx_util forest -- with bad links, self links and infectors out of range
    planted -- with random log words and random records (every code in every field, RH_DETECTED at random)"""
    hot, inf, cnt = tx_util.forest(n, pattern, seed=seed)
    return hot, inf, cnt, txlog_util.random_log(n, seed), course_util.random_records(n, seed)


def combos_state():
    """(hot, infector, n_infected, log, rec) that holds
      * as roots: RH_DETECTED set and clear x every det code and two days (one beyond N_DAYS) x o x adm x t of every code and
        days on either side of det -- every dc x ph --, n_infected at and beyond the end of the offspring histogram;
      * det - t at -1, 0, 63, 64 and 100 (at_large: one bin inside and one beyond at both ends);
      * links of every dc(s) x t(i) code and days before, on and after det(s), with det(s) - t(i) at 63 and 64 (lead), and
        infectees of every dc with det(i) - det(s) at -65, -64, -63, 0, 1, 62, 63, 64 (pair);
      * bad links: a self link, an infector out of range, a negative word that is not -1, a susceptible infector;
    scattered over a population with a few untouched agents."""
    A = []                                             # [hot, t, o, det, adm, infector (an index of A, or a special), n]
    k = 0

    def add(bit, t, o, d, adm, infector=-1, n=None):
        nonlocal k
        st, sev = 1 + k % 6, k % 5
        A.append([st | sev << 3 | bit | (k % 4) << 8, t, o, d, adm, infector, (0, 1, 62, 63, 64, 200)[k % 6] if n is None else n])
        k += 1
        return len(A) - 1

    for bit in (0, DETECTED):
        for d in (NO, BF, 120, 350):
            for o in (NO, BF, 100, 120, 130):
                for adm in (NO, BF, 110, 120, 125):
                    for t in (NO, BF, 95, 299, 300):
                        add(bit, t, o, d, adm)
    for delta in (-1, 0, 63, 64, 100):
        add(DETECTED, 200 - delta, 190, 200, NO)
    sources = [add(0, 90, 95, NO, NO), add(DETECTED, 90, 95, 200, NO), add(DETECTED, BF, BF, BF, NO), add(DETECTED, 90, 95, NO, NO),
               add(0, 90, 95, 200, 200)]             # dc 0, 1, 2, 3, and dated although RH_DETECTED is clear: the record first
    for s in sources:
        for t in (NO, BF, 150, 199, 200, 201, 137, 136, 100, N_DAYS + 5):
            add(0, t, NO, NO, NO, s)
        for bit, d in ((0, NO), (DETECTED, NO), (0, BF), (DETECTED, BF)):
            add(bit, 180, NO, d, NO, s)
        for delta in (-65, -64, -63, 0, 1, 62, 63, 64):
            add(DETECTED, 130, NO, 200 + delta, NO, s)
    susceptible = len(A)
    A.append([0, NO, NO, NO, NO, -1, 0])
    bad = [add(0, 100, NO, NO, NO, 'self'), add(0, 100, NO, 150, NO, 'beyond'), add(DETECTED, 100, NO, NO, NO, -7),
           add(0, 100, NO, NO, NO, susceptible)]
    m = len(A)
    n = m + 9
    rng = np.random.default_rng(13)
    where = rng.permutation(n)[:m]
    H = np.zeros(n, dtype=np.uint32)
    L = np.full(n, NO << 16 | NO, dtype=np.uint32)
    R = np.full(n, (1 << 64) - 1, dtype=np.uint64)
    I = np.full(n, -1, dtype=np.int32)
    C = np.zeros(n, dtype=np.int32)
    for j, (h, t, o, d, adm, src, cnt) in enumerate(A):
        i = int(where[j])
        H[i], L[i], C[i] = h, o << 16 | t, cnt
        R[i] = int(crs.pack([d], [adm], [NO], [NO])[0])
        I[i] = i if src == 'self' else (n + 3 if src == 'beyond' else (src if src < 0 else int(where[src])))
    assert len(bad) == 4
    return H, I, C, L, R


def walk_report(hot, infector, n_infected, log, rec, age_start, age_group, n_days):
    """Every field of a report, counted agent by agent and link by link in plain Python from the header's text (independent of
    report_numpy and of reports.links)"""
    n = len(hot)
    hot = [int(x) for x in np.asarray(hot, dtype=np.uint32)]
    src = [int(x) for x in np.asarray(infector, dtype=np.int32)]
    cnt = [int(x) & 0xFFFFFFFF for x in np.asarray(n_infected)]
    log = [int(x) for x in np.asarray(log, dtype=np.uint32)]
    rec = [int(x) for x in np.asarray(rec, dtype=np.uint64)]
    starts = [int(x) for x in age_start]
    nr_ages = len(age_group)
    age = lambda i: min(max(bisect.bisect_right(starts[:nr_ages + 1], i) - 1, 0), nr_ages - 1)
    known = lambda x: x not in (NO, BF)
    clip = lambda x, hi: min(max(x, 0), hi)
    ascertain = np.zeros((16, 8, 4), dtype=np.uint64)
    phase = np.zeros((16, 4), dtype=np.uint64)
    at_large = np.zeros((16, 64), dtype=np.uint64)
    at_large_n = np.zeros(16, dtype=np.uint64)
    at_large_sum = np.zeros(16, dtype=np.int64)
    offspring = np.zeros((4, 2, 64), dtype=np.uint64)
    offspring_sum = np.zeros((4, 2), dtype=np.uint64)
    link_class = np.zeros((16, 5), dtype=np.uint64)
    lead = np.zeros((16, 64), dtype=np.uint64)
    pair = np.zeros(128, dtype=np.uint64)
    pair_class = np.zeros((4, 4), dtype=np.uint64)
    cohort = np.zeros((n_days, 16, 3), dtype=np.uint64)
    detections = np.zeros((n_days, 4), dtype=np.uint64)
    links_by_day = np.zeros((n_days, 3), dtype=np.uint64)
    sc = {name: 0 for name in det.SCALAR_NAMES}

    def dclass(i):
        d = rec[i] & 0xFFFF
        if known(d):
            return 1
        if d == BF:
            return 2
        return 3 if hot[i] & DETECTED else 0

    for i in range(n):
        h = hot[i]
        st = h & 7
        if st == 0:
            continue
        g = age_group[age(i)]
        t, o = log[i] & 0xFFFF, log[i] >> 16
        d, adm = rec[i] & 0xFFFF, (rec[i] >> 16) & 0xFFFF
        dc = dclass(i)
        closed = 1 if st >= 5 else 0
        sc['infected'] += 1
        sc[det.CLASS_NAMES[dc]] += 1
        ascertain[g, (h >> 3) & 7, dc] += 1
        offspring[dc, closed, min(cnt[i], 63)] += 1
        offspring_sum[dc, closed] += cnt[i]
        ph = None
        if dc == 1:
            if o == NO or (known(o) and d < o):
                ph = 0
            elif known(adm) and d == adm:
                ph = 1
            elif known(o) and (adm == NO or (known(adm) and d < adm)):
                ph = 2
            else:
                ph = 3
            phase[g, ph] += 1
            if d < n_days:
                detections[d, ph] += 1
            else:
                sc['out_of_range'] += 1
            if known(t):
                at_large[g, clip(d - t, 63)] += 1
                at_large_n[g] += 1
                at_large_sum[g] += d - t
        if known(t):
            if t < n_days:
                cohort[t, g, 0] += 1
                cohort[t, g, 1] += dc != 0
                cohort[t, g, 2] += closed
            else:
                sc['out_of_range'] += 1
        s = src[i]
        if s == -1:
            sc['roots'] += 1
            continue
        if not (0 <= s < n) or s == i or hot[s] & 7 == 0:
            sc['bad_links'] += 1
            continue
        sc['linked'] += 1
        gs, dcs, ds = age_group[age(s)], dclass(s), rec[s] & 0xFFFF
        if dcs == 0:
            cls = 0
        elif dcs in (2, 3) or not known(t):
            cls = 4
        elif t < ds:
            cls = 1
        elif t == ds:
            cls = 2
        else:
            cls = 3
            sc['breach'] += 1
        link_class[gs, cls] += 1
        pair_class[dcs, dc] += 1
        if cls in (1, 2):
            lead[gs, clip(ds - t, 63)] += 1
        if dcs == 1 and dc == 1:
            pair[clip(d - ds + 64, 127)] += 1
        if known(t) and t < n_days:
            links_by_day[t, 0] += 1
            links_by_day[t, 1] += cls == 0
            links_by_day[t, 2] += cls in (1, 2)
    w = np.concatenate([ascertain.ravel(), phase.ravel(), at_large.ravel(), at_large_n, at_large_sum.view(np.uint64), offspring.ravel(),
                        offspring_sum.ravel(), link_class.ravel(), lead.ravel(), pair, pair_class.ravel(),
                        np.array([sc[name] for name in det.SCALAR_NAMES] + [0] * (det.S_NR - len(det.SCALAR_NAMES)), dtype=np.uint64),
                        cohort.ravel(), detections.ravel(), links_by_day.ravel()])
    assert len(w) == det.report_words(n_days)
    return w


def put_state(ctx, hot, infector, n_infected, log, rec):
    """a synthetic state into a Context's engine, a transmission log and a course begun on it: the forest through
    tx_util.put_forest, the log words and the records through the logs' own write routes"""
    tx_util.put_forest(ctx, hot, infector, n_infected)
    tlog = ctx.start_transmission_log()
    tlog.set_words(log)
    course = ctx.start_course_log()
    course.set_words(rec)
    return ctx


def host_arrays(ctx):
    """(hot, infector, n_infected) of a Context's engine, host copies (txlog_util.host_state)"""
    return txlog_util.host_state(ctx)


def spec_report(ctx, n_days=None, groups=None, log_words=None, records=None):
    """report_numpy of a Context's read-back state, its log words and its course records"""
    hot, inf, cnt = host_arrays(ctx)
    log = ctx.transmission_log.words() if log_words is None else log_words
    rec = ctx.course_log.words() if records is None else records
    return det.report_numpy(hot, inf, cnt, log, rec, ctx.age_start, ctx._tx_groups(groups)[0], max(ctx.day, 1) if n_days is None else n_days)


def host_rows(ctx):
    """(state, idx) handles for tests that count directly: reports.links of the read-back state"""
    hot, inf, _ = host_arrays(ctx)
    return hot, reports.links(hot, inf)
