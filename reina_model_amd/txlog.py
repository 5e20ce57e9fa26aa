"""A dated transmission log: the day of infection and the day of symptom onset of every agent (include/reina_txlog.h;
DESIGN.md section 6f).

The engine knows who infected whom (transmission.py) but keeps no dates.  A LOG is one uint32 per agent, owned by the log
object, outside the engine state:

    word = onset_day << 16 | infection_day        codes: NONE 0xFFFF (not yet / never), BEFORE 0xFFFE (before the log began)

Days are absolute day numbers (Context.day, < 4096).  A day is KNOWN when it is neither code.

  begin        every agent with state != 0 gets infection BEFORE; of those, the ones in state >= ILLNESS get onset BEFORE too;
               every other half word is NONE.
  record day d with w the agent's hot word after day d:  infection == NONE and state(w) != 0 -> infection = d;
               onset == NONE and state(w) >= ILLNESS -> onset = d.  Nothing is ever overwritten.
  report       between two days: the epidemic curve by date of infection, the onsets by date, the cohorts behind the case
               reproduction number, and the incubation / generation / serial / onset-to-transmission intervals of every link,
               as exact integer counts (LogReport).

`begin_numpy`, `record_numpy` and `report_numpy` are the executable specification: the library's kernels (k_txlog_begin,
k_txlog_day, k_txlog_report) compute the same words.  `run_host_driven` is the plain formulation -- iterate() and
record_numpy a day at a time, on any engine -- that the device path is tested against, and what a Context on an engine
library without the log's entry points takes.

In line lists, -1 stands for NONE and -2 for BEFORE.
"""
import collections
import ctypes

import numpy as np

from . import engine as _eng
from . import reports as _rep

TXLOG_VERSION = 1              # include/reina_txlog.h: REINA_TXLOG_VERSION
NONE, BEFORE = 0xFFFF, 0xFFFE
VARIANTS, MAX_GROUPS = 4, 16
INCUBATION_BINS, GENERATION_BINS, SERIAL_BINS, TOST_BINS, PHASES, COHORT_FIELDS = 64, 64, 128, 64, 4, 3
SERIAL_SHIFT, TOST_SHIFT = 32, 24
INCUBATION = 0
GENERATION = INCUBATION + VARIANTS * INCUBATION_BINS
SERIAL = GENERATION + VARIANTS * GENERATION_BINS
TOST = SERIAL + VARIANTS * SERIAL_BINS
LINK_PHASE = TOST + VARIANTS * TOST_BINS
SCALARS = LINK_PHASE + VARIANTS * PHASES
SCALAR_NAMES = ('infected', 'dated', 'before', 'with_onset', 'links', 'links_dated', 'generation_nonpositive', 'first_day',
                'last_day', 'out_of_range', 'bad_links')
S_NR = 16
FIXED_WORDS = SCALARS + S_NR
DAY_WORDS = VARIANTS * (MAX_GROUPS + 1 + COHORT_FIELDS)
PHASE_NAMES = ('presymptomatic', 'symptomatic', 'infector_without_onset', 'undated')
S_ILLNESS, S_RECOVERED = 2, 5   # csrc/reina_prims.h: RS_ILLNESS, RS_RECOVERED

TXLOG_FUNCTIONS = ('txlog_version', 'txlog_create', 'group_txlog_create', 'txlog_destroy', 'txlog_record_day', 'txlog_run_days',
                   'group_txlog_run_days', 'txlog_report', 'group_txlog_report', 'txlog_read', 'txlog_write')


def incidence_offset(n_days):
    return FIXED_WORDS


def onsets_offset(n_days):
    return incidence_offset(n_days) + int(n_days) * VARIANTS * MAX_GROUPS


def cohort_offset(n_days):
    return onsets_offset(n_days) + int(n_days) * VARIANTS


def report_words(n_days):
    """include/reina_txlog.h: REINA_TXLOG_REPORT_WORDS"""
    return FIXED_WORDS + int(n_days) * DAY_WORDS


def check_n_days(n_days):
    """the one statement of a report's range of days; every route takes it before it builds or launches anything"""
    if not 1 <= int(n_days) <= _eng.MAX_DAYS:
        raise ValueError('n_days must be in [1, %d]' % _eng.MAX_DAYS)
    return int(n_days)


def day_arguments(ctx, age_groups, n_days):
    """(table, labels, n_days) of a report by day: the Context's report groups, and n_days checked (default: the days run so
    far) -- the argument check of the log, course and vaccination reports"""
    table, labels = ctx._tx_groups(age_groups)
    return table, labels, check_n_days(max(int(ctx.day), 1) if n_days is None else n_days)


_vp, _u32 = ctypes.c_void_p, ctypes.c_uint32
_TXLOG_ARGTYPES = {'txlog_create': [_vp, _vp, _vp], 'group_txlog_create': [_vp, _vp, _vp], 'txlog_destroy': [_vp],
                   'txlog_record_day': [_vp, _u32, _vp],
                   'txlog_run_days': [_vp, _vp, _u32, _vp, _vp], 'group_txlog_run_days': [_vp, _vp, _u32, _vp, _vp],
                   'txlog_report': [_vp, _vp, _u32, _u32, _vp, _vp], 'group_txlog_report': [_vp, _vp, _u32, _u32, _vp, _vp],
                   'txlog_read': [_vp, _u32, _vp, _vp], 'txlog_write': [_vp, _u32, _vp, _vp]}


def bind_txlog_abi(lib, prefix):
    """The log's entry points of a library, or None when it has none."""
    return _eng.bind_optional_abi(lib, prefix, TXLOG_FUNCTIONS, _TXLOG_ARGTYPES, 'txlog_version', TXLOG_VERSION)


# ------------------------------------------------------------------------------------------------ the specification

def begin_numpy(hot):
    """the log of a state as the begin pass leaves it"""
    st = np.asarray(hot).view(np.uint32).ravel() & 7
    inf = np.where(st != 0, BEFORE, NONE).astype(np.uint32)
    ons = np.where(st >= S_ILLNESS, BEFORE, NONE).astype(np.uint32)
    return ons << 16 | inf


def record_numpy(log, hot, day):
    """`log` after day `day` has been recorded from the hot words as they stand after that day (a new array)"""
    day = int(day)
    if not 0 <= day < _eng.MAX_DAYS:
        raise ValueError('day %d: the log holds days below %d' % (day, _eng.MAX_DAYS))
    log = np.asarray(log, dtype=np.uint32).ravel()
    st = np.asarray(hot).view(np.uint32).ravel() & 7
    inf, ons = log & 0xFFFF, log >> 16
    inf = np.where((inf == NONE) & (st != 0), day, inf).astype(np.uint32)
    ons = np.where((ons == NONE) & (st >= S_ILLNESS), day, ons).astype(np.uint32)
    return ons << 16 | inf


LinkDays = collections.namedtuple('LinkDays', 'idx s linked bad w v t o tk ok ts os tsk osk both phase')


def link_days(hot, infector, log):
    """The ONE statement of what the reports of a log read of every infected agent (over idx, reports.links): its hot word w and
    variant v, its infection and onset day t / o (tk / ok: known), its infector's ts / os on a link (tsk / osk: linked and
    known), both (t and ts known) and the link phase -- 0 t < os, both known (presymptomatic); 1 t >= os, both known; 2 t known
    and os NONE; 3 anything else.  report_numpy and regime.report_numpy are built on it."""
    hot = np.asarray(hot).view(np.uint32).ravel()
    log = np.asarray(log, dtype=np.uint32).ravel()
    _, idx, s, _, linked, bad = _rep.links(hot, infector)
    w = hot[idx]
    v = ((w >> 8) & 3).astype(np.int64)
    t = (log[idx] & 0xFFFF).astype(np.int64)
    o = (log[idx] >> 16).astype(np.int64)
    tk, ok = t < BEFORE, o < BEFORE
    sl = np.zeros(len(idx), dtype=np.uint32)
    sl[linked] = log[s[linked]]
    ts, os_ = (sl & 0xFFFF).astype(np.int64), (sl >> 16).astype(np.int64)
    tsk, osk = linked & (ts < BEFORE), linked & (os_ < BEFORE)
    phase = np.where(tk & osk, np.where(t < os_, 0, 1), np.where(tk & (os_ == NONE), 2, 3))
    return LinkDays(idx, s, linked, bad, w, v, t, o, tk, ok, ts, os_, tsk, osk, tk & tsk, phase)


def report_numpy(hot, infector, n_infected, log, age_start, age_group, n_days):
    """The report of one state and its log (the specification of reina_txlog_report).  hot: uint32[N]; infector, n_infected:
    int32[N] (the cold record's fields); log: uint32[N]; age_start: first agent of each age ([A] = N, padded with N);
    age_group: group of each age (< MAX_GROUPS); n_days: the dated tables hold the days [0, n_days)."""
    hot = np.asarray(hot).view(np.uint32).ravel()
    n_days = check_n_days(n_days)
    cnt = np.asarray(n_infected).view(np.uint32).ravel().astype(np.uint64)
    table, n_groups, _, age_of = _rep.age_lookup(age_start, age_group)
    words = np.zeros(report_words(n_days), dtype=np.uint64)
    idx, s, linked, bad, w, v, t, o, tk, ok, ts, os_, tsk, osk, both, phase = link_days(hot, infector, log)

    def hist(offset, bins, sel, value):
        cell = v[sel] * bins + np.clip(value, 0, bins - 1)
        words[offset:offset + VARIANTS * bins] = np.bincount(cell, minlength=VARIANTS * bins).astype(np.uint64)

    hist(INCUBATION, INCUBATION_BINS, tk & ok, (o - t)[tk & ok])
    hist(GENERATION, GENERATION_BINS, both, (t - ts)[both])
    hist(SERIAL, SERIAL_BINS, ok & osk, (o - os_ + SERIAL_SHIFT)[ok & osk])
    hist(TOST, TOST_BINS, tk & osk, (t - os_ + TOST_SHIFT)[tk & osk])
    hist(LINK_PHASE, PHASES, linked, phase[linked])

    g = table[age_of(idx)].astype(np.int64)
    inr = tk & (t < n_days)
    a, b, c = incidence_offset(n_days), onsets_offset(n_days), cohort_offset(n_days)
    words[a:b] = np.bincount((t[inr] * VARIANTS + v[inr]) * MAX_GROUPS + g[inr], minlength=b - a).astype(np.uint64)
    onr = ok & (o < n_days)
    words[b:c] = np.bincount(o[onr] * VARIANTS + v[onr], minlength=c - b).astype(np.uint64)
    key = t[inr] * VARIANTS + v[inr]
    coh = np.zeros((n_days * VARIANTS, COHORT_FIELDS), dtype=np.uint64)
    coh[:, 0] = np.bincount(key, minlength=len(coh)).astype(np.uint64)
    np.add.at(coh[:, 1], key, cnt[idx][inr])
    coh[:, 2] = np.bincount(key[(w[inr] & 7) >= S_RECOVERED], minlength=len(coh)).astype(np.uint64)
    words[c:] = coh.ravel()
    sc = dict(infected=len(idx), dated=int(tk.sum()), before=int((t == BEFORE).sum()), with_onset=int(ok.sum()),
              links=int(linked.sum()), links_dated=int(both.sum()), generation_nonpositive=int((both & (t <= ts)).sum()),
              first_day=int(t[tk].min()) if tk.any() else (1 << 64) - 1, last_day=int(t[tk].max()) if tk.any() else 0,
              out_of_range=int((tk & (t >= n_days)).sum()) + int((ok & (o >= n_days)).sum()), bad_links=int(bad.sum()))
    for k, name in enumerate(SCALAR_NAMES):
        words[SCALARS + k] = sc[name]
    return LogReport(words, n_days, n_groups)


# ------------------------------------------------------------------------------------------------ reports

class _Intervals:
    """one interval distribution: counts by value (a pandas Series through .series()), and its mean"""

    def __init__(self, counts, shift, name):
        self.counts = np.asarray(counts, dtype=np.int64)
        self.values = np.arange(len(self.counts)) - shift
        self.name = name

    def series(self):
        import pandas as pd
        return pd.Series(self.counts, index=pd.Index(self.values, name=self.name), name='count')

    def total(self):
        return int(self.counts.sum())

    def mean(self):
        """None when empty; the end bins hold the clipped values"""
        n = self.total()
        return float((self.counts * self.values).sum()) / n if n else None

    def quantile(self, q):
        n = self.total()
        if not n:
            return None
        if not 0 <= q <= 1:
            raise ValueError('quantile: q must be in [0, 1]')
        return int(self.values[np.argmax(np.cumsum(self.counts) >= q * n)])   # (the first value the cumulated counts reach q * n at)


class LogReport(_rep.Report):
    """One report: the words of include/reina_txlog.h as named arrays, plus what is derived from them."""
    SCALARS, SCALAR_NAMES, IDENTITY = SCALARS, SCALAR_NAMES, ('n_days',)

    def __init__(self, words, n_days, n_groups=MAX_GROUPS, group_labels=None, start_date=None):
        self.n_days = n_days = int(n_days)
        w = self._take(words, report_words(n_days), 'a log report of %d days has %d words' % (n_days, report_words(n_days)),
                       n_groups, group_labels)
        self.start_date = start_date
        self.incubation = w[INCUBATION:GENERATION].reshape(VARIANTS, INCUBATION_BINS)
        self.generation = w[GENERATION:SERIAL].reshape(VARIANTS, GENERATION_BINS)
        self.serial = w[SERIAL:TOST].reshape(VARIANTS, SERIAL_BINS)
        self.tost = w[TOST:LINK_PHASE].reshape(VARIANTS, TOST_BINS)
        self.link_phase = w[LINK_PHASE:SCALARS].reshape(VARIANTS, PHASES)
        a, b, c = incidence_offset(n_days), onsets_offset(n_days), cohort_offset(n_days)
        self.incidence = w[a:b].reshape(n_days, VARIANTS, MAX_GROUPS)
        self.onsets = w[b:c].reshape(n_days, VARIANTS)
        self.cohort = w[c:].reshape(n_days, VARIANTS, COHORT_FIELDS)
        if self.dated == 0:
            self.first_day = self.last_day = -1

    def __repr__(self):
        return 'LogReport(days=%d, infected=%d, dated=%d, before=%d, links=%d)' % (self.n_days, self.infected, self.dated, self.before, self.links)

    def _v(self, arr, variant):
        """one variant's part of an array ([variant, ...] or [day, variant, ...]), or the sum over the variants"""
        axis = 0 if arr.ndim == 2 else 1
        if variant is None:
            return arr.sum(axis=axis, dtype=np.uint64)
        return np.take(arr, int(variant), axis=axis)

    def incidence_frame(self, variant=None):
        """infections by date of infection (rows) and age group (columns), of one variant or all"""
        import pandas as pd
        m = self._v(self.incidence, variant)[:, :self.n_groups].astype(np.int64)
        return pd.DataFrame(m, index=self._dates(), columns=pd.Index(self._groups(), name='age_group'))

    def onset_series(self, variant=None):
        import pandas as pd
        o = self.onsets.sum(axis=1, dtype=np.uint64) if variant is None else self.onsets[:, int(variant)]   # ([day, variant])
        return pd.Series(o.astype(np.int64), index=self._dates(), name='onsets')

    def incubation_period(self, variant=None):
        return _Intervals(self._v(self.incubation, variant), 0, 'incubation_period')

    def generation_interval(self, variant=None):
        return _Intervals(self._v(self.generation, variant), 0, 'generation_interval')

    def serial_interval(self, variant=None):
        return _Intervals(self._v(self.serial, variant), SERIAL_SHIFT, 'serial_interval')

    def onset_to_transmission(self, variant=None):
        return _Intervals(self._v(self.tost, variant), TOST_SHIFT, 'onset_to_transmission')

    def presymptomatic_share(self, variant=None):
        """links whose infectee was infected before the infector's onset, over the links where both days are known; None
        when there is none"""
        p = self._v(self.link_phase, variant)
        n = int(p[0]) + int(p[1])
        return int(p[0]) / n if n else None

    def case_reproduction_number(self, variant=None):
        """by date of infection: R_c (mean offspring of the agents infected that day so far; NaN for an empty cohort), the
        cohort's size and the share of it that is removed (R_c of an open cohort is censored)"""
        import pandas as pd
        c = self._v(self.cohort, variant).astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            rc, closed = c[:, 1] / c[:, 0], c[:, 2] / c[:, 0]
        return pd.DataFrame(dict(r_c=rc, cohort=c[:, 0].astype(np.int64), closed_share=closed), index=self._dates())


# ------------------------------------------------------------------------------------------------ logs

def check_capable(ctx):
    if ctx.n_shards != 1 or ctx.always_collective:
        raise ValueError('transmission log: sharded Contexts are refused (links are global ids, and a shard sees only its own '
                         "agents' onsets)")


def _host_array(t):
    return np.array(t.cpu().numpy() if hasattr(t, 'cpu') else t)


class DeviceLog(_eng.Handle):
    """The library's log of one engine, or of the members of an engine group (include/reina_txlog.h)."""
    DESTROY = 'txlog_destroy'

    def __init__(self, engine, group=None):
        f = _rep.entry_points(engine, 'txlog_f', 'transmission-log', 'reina_txlog.h')
        self.f, self.engine, self.group = f, engine, group
        self.members = 1 if group is None else len(group.engines)
        self.course = None   # course.DeviceCourse once one is attached: the record launches record it too
        self._h = ctypes.c_void_p()
        if group is None:
            engine._check(f['txlog_create'](engine._h, engine.alloc.stream(), ctypes.byref(self._h)), 'txlog_create')
        else:
            engine._check(f['group_txlog_create'](group._h, engine.alloc.stream(), ctypes.byref(self._h)), 'group_txlog_create')

    def _closing(self):
        if self.course is not None:
            self.course.close()

    @property
    def engines(self):
        return [self.engine] if self.group is None else self.group.engines

    def _touch(self):
        _eng.mark_stale(self.engines)

    def record_day(self, day):
        self.engine._check(self.f['txlog_record_day'](self._h, int(day), self.engine.alloc.stream()), 'txlog_record_day')

    def run_day_array(self, arr, n, history):
        """Engine.run_day_array / EngineGroup.run_day_array with the record launch behind every day"""
        if self.group is None:
            self._touch()
            self.engine._check(self.f['txlog_run_days'](self._h, arr, n, history, self.engine.alloc.stream()), 'txlog_run_days')
            return
        hp = _eng.member_pointers(self.group.engines, history)
        self.engine._check(self.f['group_txlog_run_days'](self._h, arr, n, hp, self.engine.alloc.stream()), 'group_txlog_run_days')

    def words(self, member=0):
        out = np.zeros(self.engine.config.n_agents, dtype=np.uint32)
        self.engine._check(self.f['txlog_read'](self._h, int(member), out.ctypes.data, self.engine.alloc.stream()), 'txlog_read')
        return out

    def set_words(self, words, member=0):
        w = np.ascontiguousarray(words, dtype=np.uint32)
        if len(w) != self.engine.config.n_agents:
            raise ValueError('a log has one word per agent')
        self.engine._check(self.f['txlog_write'](self._h, int(member), w.ctypes.data, self.engine.alloc.stream()), 'txlog_write')


class TransmissionLog:
    """The log of one Context (ctx.transmission_log): on the device when the engine library has the log's entry points, in
    host memory otherwise (or with host=True: the plain formulation).  A member of a logged engine group shares the group's
    DeviceLog (`device`, `member`)."""

    def __init__(self, ctx, host=False, device=None, member=0):
        check_capable(ctx)
        self.ctx, self.member = ctx, int(member)
        self.begin_day = int(ctx.day)
        self.course = None   # course.CourseLog once one is attached (Context.start_course_log)
        self.device, self._words = device, None
        if device is None:
            # (under a policy the device log needs the combined run of include/reina_regime.h: a library with the log's entry
            # points but without those keeps the log in host memory, where policy.run_host_driven records it)
            combined = ctx.policy is None or getattr(ctx.engine, 'regime_f', None) is not None
            if not host and _eng.is_device(ctx.engine) and ctx.engine.txlog_f is not None and combined:
                self.device = DeviceLog(ctx.engine)
            else:
                self._words = begin_numpy(_host_array(ctx.engine.tensors['hot']))

    @property
    def on_device(self):
        return self.device is not None

    def close(self):
        if self.device is not None and self.device.group is None:
            self.device.close()

    def record_day(self, day):
        """behind a day the caller stepped itself (Context.iterate does)"""
        if self.device is not None:
            self.device.record_day(day)
        else:
            hot = _host_array(self.ctx.engine.tensors['hot'])
            self._words = record_numpy(self._words, hot, day)
            if self.course is not None:
                self.course.record_host(hot, day)

    def words(self):
        """uint32[n_agents], a host copy"""
        return self.device.words(self.member) if self.device is not None else self._words.copy()

    def set_words(self, words):
        """replace the words (a log saved by words(), continued on the same state)"""
        if self.device is not None:
            self.device.set_words(words, self.member)
        else:
            self._words = np.array(words, dtype=np.uint32)

    def infection_day(self):
        """int64[n_agents]: the day of infection, -1 NONE, -2 BEFORE"""
        return _signed(self.words() & 0xFFFF)

    def onset_day(self):
        return _signed(self.words() >> 16)

    def report(self, age_groups=None, n_days=None):
        """LogReport of the days [0, n_days) (default: the days run so far)"""
        return _rep.report_of(LOG, self, age_groups, n_days)

    def lineage_report(self, period=7, n_periods=None, age_groups=None):
        """lineage.LineageReport between two days: who infects whom by period of `period` days, and the trees of the run by
        the period they were seeded in.  n_periods: default the periods that hold the days run so far (at most 256:
        ValueError beyond).  On the device when the library has the entry points and the log is there, lineage.report_numpy
        on host copies otherwise.  Reads the engine's state and the log only."""
        from . import lineage as _lin
        return _lin.report_log(self, period, n_periods, age_groups)

    def regime_report(self, labels=None, age_groups=None, n_days=None):
        """regime.RegimeReport: transmission by the regime in force -- intervals, presymptomatic share, age mixing, offspring
        and the links that cross a change, per regime.  labels: day -> regime 0..7 or 0xFF (regime.py), one per day of
        [0, n_days) (default: the days run so far); None takes the levels of the Context's policy runs
        (Context.policy_level_by_day; ValueError for a Context that never ran under one).  On the device when the library has
        the entry points and the log is there, regime.report_numpy on host copies otherwise.  Reads the engine's state and the
        log only."""
        from . import regime as _rgm
        return _rgm.report_log(self, labels, age_groups, n_days)

    def vaccination_report(self, age_groups=None, n_days=None):
        """vaccination.VaccinationReport of the days [0, n_days) (default: the days run so far): coverage by date and age group,
        infections by status at infection (unvaccinated, recent, protected), the time from the dose to a breakthrough, and the
        protection realised against severe disease and death.  On the device when the library has the entry points and the
        log is there, vaccination.report_numpy on host copies otherwise.  Reads the engine's state and the log only."""
        from . import vaccination as _vac
        return _vac.report_log(self, age_groups, n_days)

    def line_list(self):
        """One row per infected agent (a pandas DataFrame, built on the host from the hot words, the cold records and the log):
        agent, age, infector (-1: an import or the initial condition), infector_age (-1 without one), infection_day and
        onset_day (-1 NONE, -2 BEFORE), variant, severity, state, detected, n_infected.  The infector column holds every
        infector word that is in range, that of a bad link (a self-link, a link to a susceptible agent) included: a row has an
        infector when its word names an agent, not only when reports.links calls it linked.  With a course log attached
        (course.py): detection_day, admission_day, icu_day and outcome_day as well."""
        import pandas as pd
        hot, infector, n_infected, _ = _rep.host_state(self.ctx.engine)
        log = self.words()
        _, idx, src, _, _, _ = _rep.links(hot, infector)
        age = _rep.age_lookup(self.ctx.age_start, np.zeros(self.ctx.nr_ages, dtype=np.int64))[3]   # (the ages alone: no groups here)
        has = (src >= 0) & (src < len(hot))
        w = hot[idx]
        df = pd.DataFrame(dict(
            agent=idx, age=age(idx), infector=np.where(has, src, -1), infector_age=np.where(has, age(np.where(has, src, 0)), -1),
            infection_day=_signed(log[idx] & 0xFFFF), onset_day=_signed(log[idx] >> 16), variant=((w >> 8) & 3).astype(np.int64),
            severity=np.minimum((w >> 3) & 7, 4).astype(np.int64), state=(w & 7).astype(np.int64), detected=(w & 0x40) != 0,
            n_infected=n_infected.view(np.int32)[idx].astype(np.int64)))
        if self.course is not None:
            for name, days in zip(('detection_day', 'admission_day', 'icu_day', 'outcome_day'), self.course.days()):
                df[name] = days[idx]
        return df


def _signed(half):
    h = np.asarray(half).astype(np.int64)
    return np.where(h == NONE, -1, np.where(h == BEFORE, -2, h))


def run_host_driven(ctx, days, record_history=True, on_day=None):
    """`days` days with the log kept the plain way: per day iterate(), read the hot words back, record_numpy -- one blocking
    round trip a day, on any engine.  Begins a host-side log (ctx.transmission_log) when the Context has none.  Returns history
    like Context.run.  on_day(day, hot, log_before, log_after), when given, is called after every day (the tests' handle)."""
    log = ctx.transmission_log
    if log is None:
        log = ctx.transmission_log = TransmissionLog(ctx, host=True)
    if log.on_device:
        raise ValueError('run_host_driven: this Context keeps its log on the device')
    rows = []
    ctx.mobility_history = []
    for _ in range(days):
        if record_history:
            rows.append(ctx.engine.read_counters())
        ctx.mobility_history.append(float(ctx.contact_matrix.mobility_factor))
        d, changed = ctx._build_day(None)
        if changed:
            ctx._upload_tables()
        ctx.engine.step_day(d)
        ctx.day += 1
        hot = _host_array(ctx.engine.tensors['hot']).view(np.uint32)
        before = log._words
        log._words = record_numpy(before, hot, d.day)
        if log.course is not None:
            log.course.record_host(hot, d.day)
        if on_day is not None:
            on_day(int(d.day), hot, before, log._words)
    ctx._raise_on_problem(ctx.engine.read_counters())
    return np.stack(rows) if record_history and rows else (np.zeros((0, _eng.COUNTER_WORDS), dtype=np.int32) if record_history else None)


LOG = _rep.Kind(
    name='log_reports', of='transmission_log', arguments=day_arguments, report=LogReport, words=report_words,
    numpy=lambda ctx, log, table, params: lambda depth: report_numpy(*_rep.host_state(ctx.engine)[:3], log.words(), ctx.age_start,
                                                                      table, *params).words,
    names=('txlog_report', 'group_txlog_report'))


def report_group(device_log, contexts, age_groups=None, n_days=None):
    """The reports of every member of a logged group (or of the one engine of a device log): one launch for all members."""
    return _rep.reports_of_device(LOG, device_log, contexts, age_groups, n_days)


def attach_group(contexts, group, glog=None, course=False):
    """The txlog.DeviceLog of `group` with every member attached to it: `glog` when the members keep it already
    (reports.shared_log), otherwise a log begun here, every Context getting its TransmissionLog.  `course`: the group's course log
    too, begun here unless the log has one, every Context getting its CourseLog."""
    if glog is None:
        for c in contexts:
            check_capable(c)
        glog = DeviceLog(contexts[0].engine, group=group)
        for m, c in enumerate(contexts):
            c.transmission_log = TransmissionLog(c, device=glog, member=m)
    if course and glog.course is None:
        from . import course as _crs
        if any(c.course_log is not None for c in contexts):
            raise ValueError("run_group_plan: the members' course logs are not those of this group")
        gcourse = _crs.DeviceCourse(glog)
        for m, c in enumerate(contexts):
            c.course_log = _crs.CourseLog(c, device=gcourse, member=m)
    return glog
