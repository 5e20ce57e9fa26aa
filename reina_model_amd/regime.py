"""The regime report: transmission by the level in force (include/reina_regime.h).

A policy (policy.py) moves a run up and down a ladder of levels; the transmission log (txlog.py) dates every infection.  The
log's own report is by date or over the whole run.  What is a sum by date -- infections, the cohorts behind R_c -- can be joined
with the levels on the host afterwards; what is kept per LINK cannot: the generation, serial and onset-to-transmission
intervals, the presymptomatic share, who infects whom by age, the offspring distribution, and the links that cross a change
of level.  This report takes one more pass over the links with the table day -> regime at hand.

LABELS: uint8[n_days], day -> regime 0..7 (MAX_REGIMES = policy.MAX_LEVELS), or NO_REGIME (0xFF) for a day without one.  The
report does not care where they come from: a policy run's levels (Context.policy_level_by_day, the default), or the stretches
of a dated run's interventions (labels_by_value(ctx.mobility_history)).  The SLOT of a day d is labels[d] when d is a known day
(txlog: neither NONE nor BEFORE), d < n_days and labels[d] < 8, and slot 8 otherwise -- a day before the log began, a day
beyond n_days, an unlabelled day.

t, o (infection and onset day of the log word), v (variant), g (age group), linked, bad and the link phase are those of
txlog.report_numpy and reports.links.  With i an infected agent, s its infector on a link, r = slot(t(i)) the regime at
transmission:

  days[9]               the days d in [0, n_days) by slot
  infections[9][4][16]  infected agents by (slot(t(i)), v, g)
  cohort[9][4][3]       by (slot(t(i)), v): agents, the sum of their n_infected, those removed (state >= RECOVERED)
  offspring[9][32]      removed agents (closed cases) by (slot(t(i)), min(n_infected, 31))
  generation[9][64]     links with both days known by (r, t(i) - t(s) clipped)
  serial[9][128]        links with both onsets known by (r, o(i) - o(s) + 32 clipped)
  tost[9][64]           links with t(i) and o(s) known by (r, t(i) - o(s) + 24 clipped)
  link_phase[9][4]      every link by (r, phase)
  crossing[9][9]        every link by (slot(t(s)), slot(t(i)))
  mixing[9][16][16]     every link by (r, g(s), g(i))
  scalars               infected, dated, in_range, unlabelled, links, links_dated, links_crossing, bad_links

`report_numpy` is the executable specification, over all agents: the library's kernel (k_regime_report) computes the same
words.  A report is a function of the state, the log and the labels alone, so the host route -- report_numpy on host copies,
what oracle B, a host-kept log and a group's member taken alone take -- and the device route agree word for word.
"""
import collections
import ctypes

import numpy as np

from . import engine as _eng
from . import reports as _rep
from . import txlog as _txl
from .txlog import SERIAL_SHIFT, TOST_SHIFT, S_RECOVERED, check_n_days

REGIME_VERSION = 1             # include/reina_regime.h: REINA_REGIME_VERSION
MAX_REGIMES, NO_REGIME = 8, 0xFF
SLOTS = MAX_REGIMES + 1
MAX_GROUPS, VARIANTS, COHORT_FIELDS, OFFSPRING_BINS = 16, 4, 3, 32
GENERATION_BINS, SERIAL_BINS, TOST_BINS, PHASES = _txl.GENERATION_BINS, _txl.SERIAL_BINS, _txl.TOST_BINS, _txl.PHASES
DAYS = 0
INFECTIONS = DAYS + SLOTS
COHORT = INFECTIONS + SLOTS * VARIANTS * MAX_GROUPS
OFFSPRING = COHORT + SLOTS * VARIANTS * COHORT_FIELDS
GENERATION = OFFSPRING + SLOTS * OFFSPRING_BINS
SERIAL = GENERATION + SLOTS * GENERATION_BINS
TOST = SERIAL + SLOTS * SERIAL_BINS
LINK_PHASE = TOST + SLOTS * TOST_BINS
CROSSING = LINK_PHASE + SLOTS * PHASES
MIXING = CROSSING + SLOTS * SLOTS
SCALARS = MIXING + SLOTS * MAX_GROUPS * MAX_GROUPS
SCALAR_NAMES = ('infected', 'dated', 'in_range', 'unlabelled', 'links', 'links_dated', 'links_crossing', 'bad_links')
REPORT_WORDS = SCALARS + len(SCALAR_NAMES)
assert REPORT_WORDS == 5714
SLOT_NAMES = tuple(str(k) for k in range(MAX_REGIMES)) + ('none',)

REGIME_FUNCTIONS = ('regime_version', 'policy_txlog_run_days', 'group_policy_txlog_run_days', 'regime_report', 'group_regime_report')
_vp, _u32 = ctypes.c_void_p, ctypes.c_uint32
_REGIME_ARGTYPES = {'policy_txlog_run_days': [_vp, _vp, ctypes.POINTER(_eng.Day), _u32, _vp, _vp],
                    'group_policy_txlog_run_days': [_vp, _vp, ctypes.POINTER(_eng.Day), _u32, ctypes.POINTER(_vp), _vp],
                    'regime_report': [_vp, _vp, _u32, _u32, _vp, _vp, _vp], 'group_regime_report': [_vp, _vp, _u32, _u32, _vp, _vp, _vp]}


def bind_regime_abi(lib, prefix):
    """The entry points of include/reina_regime.h of a library, or None when it has none."""
    return _eng.bind_optional_abi(lib, prefix, REGIME_FUNCTIONS, _REGIME_ARGTYPES, 'regime_version', REGIME_VERSION)


def report_words(n_days=None, labels=None):
    """include/reina_regime.h: REINA_REGIME_REPORT_WORDS (the block holds no table by day)"""
    return REPORT_WORDS


# ------------------------------------------------------------------------------------------------ labels

def check_labels(labels, n_days):
    """uint8[n_days] of one member's labels: a sequence of at least n_days integers, each 0..7 or NO_REGIME.  The one statement
    of what a label is; every route takes it before anything is uploaded."""
    n_days = check_n_days(n_days)
    a = np.asarray(labels)
    if a.ndim != 1 or len(a) < n_days:
        raise ValueError('labels: one label per day is wanted, %d of them' % n_days)
    if a.dtype.kind not in 'iu':
        raise ValueError('labels: integers are wanted (regimes 0..%d, or 0x%X for none)' % (MAX_REGIMES - 1, NO_REGIME))
    a = a[:n_days].astype(np.int64)
    if ((a != NO_REGIME) & ((a < 0) | (a >= MAX_REGIMES))).any():
        raise ValueError('labels: a label is a regime 0..%d, or 0x%X for none' % (MAX_REGIMES - 1, NO_REGIME))
    return a.astype(np.uint8)


def labels_by_value(seq):
    """(labels uint8[len(seq)], values): the days of any per-day sequence labelled by its distinct values in the order they first
    appear -- labels[d] = values.index(seq[d]).  Of a dated run's Context.mobility_history: the stretches of its mobility
    interventions.  ValueError above MAX_REGIMES distinct values."""
    values, labels = [], []
    for x in seq:
        if x not in values:
            if len(values) == MAX_REGIMES:
                raise ValueError('labels_by_value: more than %d distinct values' % MAX_REGIMES)
            values.append(x)
        labels.append(values.index(x))
    return np.asarray(labels, dtype=np.uint8), values


def policy_labels(ctx, n_days):
    """uint8[n_days] from Context.policy_level_by_day: the level of every day run under a policy, NO_REGIME elsewhere"""
    by_day = getattr(ctx, 'policy_level_by_day', None)
    if by_day is None or not (np.asarray(by_day) >= 0).any():
        raise ValueError('regime_report: this Context never ran under a policy -- give the labels (regime.labels_by_value)')
    lv = np.asarray(by_day, dtype=np.int64)[:n_days]
    return np.where(lv < 0, NO_REGIME, lv).astype(np.uint8)


def slots_of(days, known, labels, n_days):
    """the slot of every day of `days` (int64), `known` where the day is neither code"""
    lab = np.full(max(int(n_days), 1), NO_REGIME, dtype=np.int64)
    lab[:n_days] = np.asarray(labels, dtype=np.int64)[:n_days]
    in_range = known & (days < n_days)
    r = lab[np.where(in_range, days, 0)]
    return np.where(in_range & (r < MAX_REGIMES), r, MAX_REGIMES)


# ------------------------------------------------------------------------------------------------ the specification

def report_numpy(hot, infector, n_infected, log, age_start, age_group, labels, n_days):
    """The report of one state, its log and one member's labels (the specification of reina_regime_report).  hot, infector,
    n_infected, log, age_start, age_group: as txlog.report_numpy; labels: check_labels; n_days: the days [0, n_days) have
    labels."""
    hot = np.asarray(hot).view(np.uint32).ravel()
    n_days = check_n_days(n_days)
    labels = check_labels(labels, n_days)
    cnt = np.asarray(n_infected).view(np.uint32).ravel().astype(np.uint64)
    table, n_groups, _, age_of = _rep.age_lookup(age_start, age_group)
    words = np.zeros(REPORT_WORDS, dtype=np.uint64)
    count = lambda cells, size: np.bincount(cells, minlength=size).astype(np.uint64)
    idx, s, linked, bad, w, v, t, o, tk, ok, ts, os_, tsk, osk, both, phase = _txl.link_days(hot, infector, log)
    g = table[age_of(idx)].astype(np.int64)
    gs = np.zeros(len(idx), dtype=np.int64)
    gs[linked] = table[age_of(s[linked])]
    r, rs = slots_of(t, tk, labels, n_days), slots_of(ts, tsk, labels, n_days)
    closed = (w & 7) >= S_RECOVERED
    n = cnt[idx]

    words[DAYS:INFECTIONS] = count(slots_of(np.arange(n_days), np.ones(n_days, dtype=bool), labels, n_days), SLOTS)
    cv = r * VARIANTS + v
    words[INFECTIONS:COHORT] = count(cv * MAX_GROUPS + g, COHORT - INFECTIONS)
    coh = np.zeros((SLOTS * VARIANTS, COHORT_FIELDS), dtype=np.uint64)
    coh[:, 0] = count(cv, len(coh))
    np.add.at(coh[:, 1], cv, n)
    coh[:, 2] = count(cv[closed], len(coh))
    words[COHORT:OFFSPRING] = coh.ravel()
    words[OFFSPRING:GENERATION] = count((r * OFFSPRING_BINS + np.minimum(n, OFFSPRING_BINS - 1).astype(np.int64))[closed], GENERATION - OFFSPRING)

    def hist(offset, bins, sel, value):
        words[offset:offset + SLOTS * bins] = count(r[sel] * bins + np.clip(value[sel], 0, bins - 1), SLOTS * bins)

    hist(GENERATION, GENERATION_BINS, both, t - ts)
    hist(SERIAL, SERIAL_BINS, ok & osk, o - os_ + SERIAL_SHIFT)
    hist(TOST, TOST_BINS, tk & osk, t - os_ + TOST_SHIFT)
    hist(LINK_PHASE, PHASES, linked, phase)
    words[CROSSING:MIXING] = count((rs * SLOTS + r)[linked], SLOTS * SLOTS)
    words[MIXING:SCALARS] = count(((r * MAX_GROUPS + gs) * MAX_GROUPS + g)[linked], SCALARS - MIXING)
    in_range = tk & (t < n_days)
    sc = dict(infected=len(idx), dated=int(tk.sum()), in_range=int(in_range.sum()), unlabelled=int((in_range & (r == MAX_REGIMES)).sum()),
              links=int(linked.sum()), links_dated=int(both.sum()),
              links_crossing=int((linked & (r < MAX_REGIMES) & (rs < MAX_REGIMES) & (r != rs)).sum()), bad_links=int(bad.sum()))
    for k, name in enumerate(SCALAR_NAMES):
        words[SCALARS + k] = sc[name]
    return RegimeReport(words, n_days, labels, n_groups)


# ------------------------------------------------------------------------------------------------ reports

Offspring = collections.namedtuple('Offspring', 'counts cases mean dispersion_k')


def _slot(regime):
    """the slot of a regime argument: 0..7, or 'none' / 8 for the slot of the days without one"""
    k = MAX_REGIMES if regime == 'none' else int(regime)
    if not 0 <= k < SLOTS:
        raise ValueError('regime: 0..%d, or %r' % (MAX_REGIMES - 1, 'none'))
    return k


class RegimeReport(_rep.Report):
    """One report: the words of include/reina_regime.h as named arrays, plus what is derived from them.  `regime` arguments:
    a regime 0..7, 'none' for the slot of the days without one, or None for all slots together.  labels: the labels the report
    was taken with (uint8[n_days]), kept for the reader."""
    SCALARS, SCALAR_NAMES, IDENTITY = SCALARS, SCALAR_NAMES, ('n_days',)

    def __init__(self, words, n_days, labels=None, n_groups=MAX_GROUPS, group_labels=None, start_date=None):
        self.n_days = n_days = int(n_days)
        w = self._take(words, REPORT_WORDS, 'a regime report has %d words' % REPORT_WORDS, n_groups, group_labels)
        self.start_date = start_date
        self.labels = None if labels is None else np.asarray(labels, dtype=np.uint8)
        self.days = w[DAYS:INFECTIONS]
        self.infections = w[INFECTIONS:COHORT].reshape(SLOTS, VARIANTS, MAX_GROUPS)
        self.cohort = w[COHORT:OFFSPRING].reshape(SLOTS, VARIANTS, COHORT_FIELDS)
        self.offspring_counts = w[OFFSPRING:GENERATION].reshape(SLOTS, OFFSPRING_BINS)
        self.generation = w[GENERATION:SERIAL].reshape(SLOTS, GENERATION_BINS)
        self.serial = w[SERIAL:TOST].reshape(SLOTS, SERIAL_BINS)
        self.tost = w[TOST:LINK_PHASE].reshape(SLOTS, TOST_BINS)
        self.link_phase = w[LINK_PHASE:CROSSING].reshape(SLOTS, PHASES)
        self.crossing = w[CROSSING:MIXING].reshape(SLOTS, SLOTS)
        self.mixing = w[MIXING:SCALARS].reshape(SLOTS, MAX_GROUPS, MAX_GROUPS)

    def __repr__(self):
        return 'RegimeReport(days=%d, infected=%d, in_range=%d, unlabelled=%d, links=%d, crossing=%d)' % (
            self.n_days, self.infected, self.in_range, self.unlabelled, self.links, self.links_crossing)

    @staticmethod
    def _index():
        import pandas as pd
        return pd.Index(SLOT_NAMES, name='regime')

    def _of(self, table, regime):
        """one slot's part of a [slot, ...] table, or the sum over the slots"""
        return table.sum(axis=0, dtype=np.uint64) if regime is None else table[_slot(regime)]

    def infections_frame(self):
        """infected agents by the regime they were infected under (rows) and age group (columns), the variants together"""
        import pandas as pd
        m = self.infections.sum(axis=1, dtype=np.uint64)[:, :self.n_groups].astype(np.int64)
        return pd.DataFrame(m, index=self._index(), columns=pd.Index(self._groups(), name='age_group'))

    def reproduction_number(self):
        """per regime: R_c (the mean offspring so far of the agents infected under it; NaN for an empty cohort), the cohort's
        size, the share of it that is removed (R_c of an open cohort is censored) and the days the regime held"""
        import pandas as pd
        c = self.cohort.sum(axis=1, dtype=np.uint64).astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            rc, closed = c[:, 1] / c[:, 0], c[:, 2] / c[:, 0]
        return pd.DataFrame(dict(r_c=rc, cohort=c[:, 0].astype(np.int64), closed_share=closed, days=self.days.astype(np.int64)), index=self._index())

    def generation_interval(self, regime=None):
        return _txl._Intervals(self._of(self.generation, regime), 0, 'generation_interval')

    def serial_interval(self, regime=None):
        return _txl._Intervals(self._of(self.serial, regime), SERIAL_SHIFT, 'serial_interval')

    def onset_to_transmission(self, regime=None):
        return _txl._Intervals(self._of(self.tost, regime), TOST_SHIFT, 'onset_to_transmission')

    def presymptomatic_share(self):
        """per regime at transmission: links whose infectee was infected before the infector's onset, over the links where
        both days are known (NaN where there is none)"""
        import pandas as pd
        p = self.link_phase.astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            share = p[:, 0] / (p[:, 0] + p[:, 1])
        return pd.Series(share, index=self._index(), name='presymptomatic_share')

    def mixing_frame(self, regime=None):
        """links by the infector's age group (rows) and the infectee's (columns), of the transmissions under one regime or all"""
        import pandas as pd
        m = self._of(self.mixing, regime)[:self.n_groups, :self.n_groups].astype(np.int64)
        return pd.DataFrame(m, index=pd.Index(self._groups(), name='infector'), columns=pd.Index(self._groups(), name='infectee'))

    def crossing_frame(self):
        """links by the regime the infector was infected under (rows) and the regime at transmission (columns)"""
        import pandas as pd
        return pd.DataFrame(self.crossing.astype(np.int64), index=self._index().rename('infector'), columns=self._index().rename('infectee'))

    def offspring(self, regime=None):
        """Offspring(counts, cases, mean, dispersion_k) of the CLOSED cases infected under one regime or all: counts by
        n_infected (the last bin holds 31 and more, taken as 31), their number, the mean, and the negative-binomial dispersion
        by the method of moments, mean^2 / (var - mean) with the population variance, as TransmissionReport.dispersion_k --
        None when var <= mean, both None without a case"""
        counts = self._of(self.offspring_counts, regime).astype(np.int64)
        n = int(counts.sum())
        if not n:
            return Offspring(counts, 0, None, None)
        k = np.arange(OFFSPRING_BINS, dtype=np.int64)
        s, q = int((counts * k).sum()), int((counts * k * k).sum())
        m, var = s / n, (q * n - s * s) / (n * n)
        return Offspring(counts, n, m, m * m / (var - m) if var > m else None)


# ------------------------------------------------------------------------------------------------ routes

def _arguments(ctx, labels, age_groups, n_days):
    """(table, group labels, n_days, labels[members, n_days]): the checked arguments of a report; `labels` one row per member"""
    table, group_labels, n_days = _txl.day_arguments(ctx, age_groups, n_days)
    return table, group_labels, n_days, np.stack([check_labels(row, n_days) for row in labels])


def _numpy_route(ctx, tlog, table, params):
    n_days, labels = params
    return lambda depth: report_numpy(*_rep.host_state(ctx.engine)[:3], tlog.words(), ctx.age_start, table, labels, n_days).words


REGIME = _rep.Kind(
    name='regime_reports', of='transmission_log', arguments=_arguments, report=RegimeReport, words=report_words, numpy=_numpy_route,
    names=('regime_report', 'group_regime_report'), entry=('regime_f', 'regime-report', 'reina_regime.h'), arrays=1)


def _days(ctx, n_days):
    return check_n_days(max(int(ctx.day), 1) if n_days is None else n_days)


def _labels_of(ctx, labels, n_days):
    return policy_labels(ctx, n_days) if labels is None else check_labels(labels, n_days)


def device_report_words(device_log, table, n_groups, n_days, labels):
    """[members, REPORT_WORDS] uint64 of a txlog.DeviceLog: one launch for all members; labels [members, n_days]"""
    return _rep.device_take(REGIME, device_log, table, n_groups, (n_days, labels))()


def report_log(tlog, labels=None, age_groups=None, n_days=None):
    """TransmissionLog.regime_report (reports.report_of)"""
    n = _days(tlog.ctx, n_days)
    return _rep.report_of(REGIME, tlog, [_labels_of(tlog.ctx, labels, n)], age_groups, n)


def report_contexts(contexts, labels=None, age_groups=None, n_days=None):
    """The reports of a list of Contexts between the same two days, each member with labels of its own (labels: one sequence
    per Context, or None: every Context's policy_level_by_day): ONE launch when they are the whole of one logged group in
    member order and the library has the entry points, one by one otherwise."""
    contexts = list(contexts)
    if any(c.transmission_log is None for c in contexts):
        raise ValueError('regime_reports: a context keeps no transmission log')
    if labels is not None and len(labels) != len(contexts):
        raise ValueError('regime_reports: one sequence of labels per context is wanted')
    n = _days(contexts[0], n_days)
    rows = [_labels_of(c, None if labels is None else labels[m], n) for m, c in enumerate(contexts)]
    glog = _rep.group_log(contexts)
    if _rep._launches(REGIME, glog):
        return _rep.reports_of_device(REGIME, glog, contexts, rows, age_groups, n)
    return [_rep.report_of(REGIME, c.transmission_log, [row], age_groups, n) for c, row in zip(contexts, rows)]
