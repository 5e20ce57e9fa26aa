"""Test-side helpers of the clinical course log (reina_model_amd/course.py): synthetic states with records of every code
combination, a plain per-agent walker that counts every field of a report directly, and the scenarios of the simulated runs.

A synthetic state is NOT one a simulation could reach; it only ever goes through a report or one record launch.  Never step a
day on one."""
import bisect

import numpy as np

import tx_util
from filter_util import small_scenario
from tx_util import assert_words  # noqa: F401  (course_util.assert_words: the one of every report util)
from reina_model_amd import course as crs
from reina_model_amd import txlog as txl

N_DAYS = 300                       # the synthetic reports' n_days: some of their known days lie beyond
ACTIVE, DETECTED, POD_OUTSIDE = 0x8000, 0x40, 0x800
FIELD_VALUES = (txl.NONE, txl.BEFORE, 120, 350)   # NONE, BEFORE, a day below N_DAYS, a day beyond it
IPC = dict(dead=2, in_icu=1, in_ward=3, confirmed_cases=20, infected_cases=40, incubating=15, ill=10, recovered=10)   # tests/test_snapshot.py's


def tracing_scenario():
    """small_scenario() with everyone with symptoms tested from the start and contact tracing at full efficiency from day 20:
    the tracers queue infectees that have recovered already, so detections arrive behind closed records"""
    v, ages = small_scenario()
    v['interventions'] = [iv for iv in v['interventions'] if not iv[0].startswith('test-')] + \
        [['test-all-with-symptoms', '2020-02-18'], ['test-with-contact-tracing', '2020-03-09', 100]]
    return v, ages


def random_records(n, seed=0, top=400):
    """records of every code combination: each field NONE, BEFORE or a day in [0, top), a third each"""
    rng = np.random.default_rng([n, seed, 91])

    def field():
        kind = rng.integers(0, 3, size=n)
        day = rng.integers(0, top, size=n)
        return np.where(kind == 0, txl.NONE, np.where(kind == 1, txl.BEFORE, day))

    return crs.pack(field(), field(), field(), field())


def forest_state(n, seed=0):
    """(hot, infector, n_infected, log, rec): a random tx_util forest with random log words and records"""
    hot, inf, cnt = tx_util.forest(n, 'random', seed=seed)
    import txlog_util
    return hot, inf, cnt, txlog_util.random_log(n, seed), random_records(n, seed)


def combos_state():
    """(hot, infector, n_infected, log, rec): one agent for every state 0..6 x RH_DETECTED x each of the four fields in
    FIELD_VALUES (7 * 2 * 256 agents), some of them ACTIVE, some dead ones with RH_POD_OUTSIDE; log words with a known onset for
    most and every code now and then; and pairs of days at, and one beyond, both ends of every delay histogram"""
    hot, log, rec = [], [], []
    k = 0
    for st in range(7):
        for det_bit in (0, DETECTED):
            for det in FIELD_VALUES:
                for adm in FIELD_VALUES:
                    for icu in FIELD_VALUES:
                        for out in FIELD_VALUES:
                            hot.append(st | det_bit | (k % 4) << 8 | (ACTIVE if k % 3 else 0) | (POD_OUTSIDE if k % 5 == 0 else 0))
                            o = (100, txl.NONE, txl.BEFORE, 118, 330)[k % 5]
                            t = (95, txl.BEFORE, txl.NONE, 299, 300)[k % 7 % 5]
                            log.append(o << 16 | t)
                            rec.append((det, adm, icu, out))
                            k += 1
    N = txl.NONE
    for st in (5, 6):
        for d in (-20, -17, -16, -15, 0, 46, 47, 48, 90):          # kind 0: det - o + 16
            hot.append(st | DETECTED), log.append(200 << 16 | 190), rec.append((200 + d, N, N, N))
        for d in (-3, 0, 1, 62, 63, 64, 150):                       # every other kind: at and beyond both ends
            hot.append(st), log.append(200 << 16 | 190), rec.append((N, 200 + d, N, 200 + d + d))         # 1, 3 / 4, 7
            hot.append(st), log.append(N << 16 | 190), rec.append((N, 200, 200 + d, 200 + d + d))         # 2, 5 / 6
    n = len(hot) + 9
    rng = np.random.default_rng(11)
    where = rng.permutation(n)[:len(hot)]
    H = np.zeros(n, dtype=np.uint32)
    L = np.full(n, txl.NONE << 16 | txl.NONE, dtype=np.uint32)
    R = np.full(n, (1 << 64) - 1, dtype=np.uint64)
    H[where] = np.array(hot, dtype=np.uint32)
    L[where] = np.array(log, dtype=np.uint32)
    f = np.array(rec, dtype=np.int64)
    R[where] = crs.pack(f[:, 0], f[:, 1], f[:, 2], f[:, 3])
    return H, np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32), L, R


def walk_report(hot, log, rec, age_start, age_group, n_days):
    """Every field of a report, counted agent by agent in plain Python (independent of report_numpy)"""
    n = len(hot)
    hot = [int(x) for x in np.asarray(hot, dtype=np.uint32)]
    log = [int(x) for x in np.asarray(log, dtype=np.uint32)]
    rec = [int(x) for x in np.asarray(rec, dtype=np.uint64)]
    starts = [int(x) for x in age_start]
    nr_ages = len(age_group)
    age = lambda i: min(max(bisect.bisect_right(starts[:nr_ages + 1], i) - 1, 0), nr_ages - 1)
    known = lambda x: x not in (txl.NONE, txl.BEFORE)
    delay = np.zeros((8, 16, 64), dtype=np.uint64)
    delay_n = np.zeros((8, 16), dtype=np.uint64)
    delay_sum = np.zeros((8, 16), dtype=np.int64)
    pathway = np.zeros((16, 10), dtype=np.uint64)
    tables = np.zeros((5, n_days, 16), dtype=np.uint64)
    cohort = np.zeros((n_days, 16, 4), dtype=np.uint64)
    sc = {name: 0 for name in crs.SCALAR_NAMES}

    def add(kind, g, value):
        delay[kind, g, min(max(value, 0), 63)] += 1
        delay_n[kind, g] += 1
        delay_sum[kind, g] += value

    for i in range(n):
        h = hot[i]
        st = h & 7
        if st == 0:
            continue
        g = age_group[age(i)]
        t, o = log[i] & 0xFFFF, log[i] >> 16
        det, adm, icu, out = rec[i] & 0xFFFF, (rec[i] >> 16) & 0xFFFF, (rec[i] >> 32) & 0xFFFF, rec[i] >> 48
        sc['infected'] += 1
        for name, f in (('with_detection', det), ('with_admission', adm), ('with_icu', icu), ('with_outcome', out)):
            if known(f):
                sc[name] += 1
                if f >= n_days:
                    sc['out_of_range'] += 1
        if h & DETECTED and det == txl.NONE:
            sc['detected_undated'] += 1
        if st == 6 and h & POD_OUTSIDE:
            sc['died_outside'] += 1
        if known(det) and known(o):
            add(0, g, det - o + 16)
        if known(adm) and known(o):
            add(1, g, adm - o)
        if known(icu) and known(adm):
            add(2, g, icu - adm)
        if known(out) and known(adm) and icu == txl.NONE and st in (5, 6):
            add(3 if st == 5 else 4, g, out - adm)
        if known(out) and known(icu) and st in (5, 6):
            add(5 if st == 5 else 6, g, out - icu)
        if known(out) and known(o) and st == 6:
            add(7, g, out - o)
        if txl.BEFORE in (adm, icu, out) or (out != txl.NONE and st < 5):
            cls = 9
        else:
            cls = (0 if out == txl.NONE else (3 if st == 5 else 6)) + (2 if icu != txl.NONE else (1 if adm != txl.NONE else 0))
        pathway[g, cls] += 1
        for k, f in enumerate((det, adm, icu)):
            if known(f) and f < n_days:
                tables[k, f, g] += 1
        if known(out) and out < n_days and st in (5, 6):
            tables[3 if st == 6 else 4, out, g] += 1
        if known(t) and t < n_days:
            cohort[t, g, 0] += 1
            cohort[t, g, 1] += st >= 5
            cohort[t, g, 2] += known(adm)
            cohort[t, g, 3] += st == 6
    w = np.concatenate([delay.ravel(), delay_n.ravel(), delay_sum.view(np.uint64).ravel(), pathway.ravel(),
                        np.array([sc[name] for name in crs.SCALAR_NAMES] + [0] * (crs.S_NR - len(crs.SCALAR_NAMES)), dtype=np.uint64),
                        tables.ravel(), cohort.ravel()])
    assert len(w) == crs.report_words(n_days)
    return w


def cut_records(full, cut, hot_at_cut):
    """the records a course begun after `cut` days (hot_at_cut: the hot words then) holds at the end of the run whose full
    course is `full`, by the begin table: an agent removed by then is BEFORE throughout; otherwise a field dated before the cut
    is BEFORE -- except a detection, which the begin pass sees only through RH_DETECTED, as it does"""
    st = np.asarray(hot_at_cut).view(np.uint32) & 7
    det, adm, icu, out = crs.fields(full)
    closed = st >= 5
    f = lambda x: np.where(closed | (x < cut), txl.BEFORE, x)
    return crs.pack(f(det), f(adm), f(icu), np.where(closed, txl.BEFORE, out))
