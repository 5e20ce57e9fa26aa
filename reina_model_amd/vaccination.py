"""A vaccination report: coverage by date and age group, breakthrough infections by the time since the dose, and the protection
a programme realised against severe disease and death (include/reina_vaccination.h).

The engine stamps every vaccinated agent's day of vaccination (the cold record's vacc_day) and the flag VACCINATED in its hot
word, and an agent infected more than 14 days after its dose draws its severity with the reference's factor 0.1.  The
transmission log (txlog.py) dates every infection.  A report joins the two, between two days, and changes nothing.  With w an
agent's hot word, st = w & 7, vac = w & 0x2000, inf = st != 0, sev = (w >> 3) & 7 (drawn at infection, never cleared), vd its
vacc_day (VALID in [0, 4096)) and t the log's infection day (KNOWN when it is neither code):

  status at infection   0 unvaccinated  not vac; or vac, vd valid, t known and vd > t (vaccinated AFTER the infection: the
                                        reference vaccinates undetected infected and recovered people; scalar after_infection)
                        1 recent        vac, vd valid, t known, 0 <= t - vd <= 14
                        2 protected     vac, vd valid, t known, t - vd > 14: exactly the infections whose severity was drawn
                                        with the factor 0.1
                        3 undetermined  vac and t not known (infected before the log began), or vd not valid (scalar
                                        bad_vacc_day, which counts every vac agent with such a vd: 0 in a simulated state)

`report_numpy` is the executable specification, over all agents: the library's kernel (k_vacc_report) computes the same words.
A report is a function of the state and the log alone, so the host route -- report_numpy on host copies, what oracle B and a
host-kept log take -- and the device route agree word for word.

Protection here is REALISED protection against severe disease and death among the infected.  The model gives none against
infection (the reference: "FIXME: Change if vaccination changes transmission"), so there is no person-time at risk here.
"""
import collections
import ctypes

import numpy as np

from . import engine as _eng
from . import reports as _rep
from . import txlog as _txl
from .reports import _group_table
from .txlog import BEFORE, check_n_days

VACC_VERSION = 1               # include/reina_vaccination.h: REINA_VACC_VERSION
MAX_GROUPS, STATUSES, DATED_STATUSES, PROTECTION_DAYS, SEVERITIES = 16, 4, 3, 14, 8
OUTCOME_FIELDS, SINCE_KINDS, SINCE_BINS, POPULATION_FIELDS, COHORT_FIELDS = 4, 2, 128, 3, 4
UNVACCINATED, RECENT, PROTECTED, UNDETERMINED = 0, 1, 2, 3
SEVERITY = 0
OUTCOME = SEVERITY + STATUSES * MAX_GROUPS * SEVERITIES
SINCE = OUTCOME + STATUSES * MAX_GROUPS * OUTCOME_FIELDS
POPULATION = SINCE + SINCE_KINDS * MAX_GROUPS * SINCE_BINS
SCALARS = POPULATION + MAX_GROUPS * POPULATION_FIELDS
SCALAR_NAMES = ('vaccinated', 'infected', 'vaccinated_infected', 'after_infection', 'undetermined', 'bad_vacc_day', 'out_of_range')
S_NR = 16
FIXED_WORDS = SCALARS + S_NR
DAY_WORDS = MAX_GROUPS * (1 + DATED_STATUSES) + DATED_STATUSES * COHORT_FIELDS
STATUS_NAMES = ('unvaccinated', 'recent', 'protected', 'undetermined')
SEVERITY_NAMES = ('asymptomatic', 'mild', 'severe', 'critical', 'fatal', '5', '6', '7')
OUTCOME_NAMES = ('agents', 'closed', 'dead', 'detected')
POPULATION_NAMES = ('vaccinated', 'susceptible', 'infected')
COHORT_NAMES = ('agents', 'severe', 'dead', 'closed')
V_SEVERE = 2                                   # csrc/reina_prims.h: RV_SEVERE
S_RECOVERED, S_DEAD = 5, 6                     # csrc/reina_prims.h: RS_*
H_DETECTED, H_VACCINATED = 0x40, 0x2000        # csrc/reina_prims.h: RH_*

VACC_FUNCTIONS = ('vacc_version', 'vacc_report')


def vaccinations_offset(n_days):
    return FIXED_WORDS


def infections_offset(n_days):
    return vaccinations_offset(n_days) + int(n_days) * MAX_GROUPS


def cohort_offset(n_days):
    return infections_offset(n_days) + int(n_days) * MAX_GROUPS * DATED_STATUSES


def report_words(n_days):
    """include/reina_vaccination.h: REINA_VACC_REPORT_WORDS"""
    return FIXED_WORDS + int(n_days) * DAY_WORDS


def bind_vacc_abi(lib, prefix):
    """The vaccination report's entry points of a library, or None when it has none."""
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    return _eng.bind_optional_abi(lib, prefix, VACC_FUNCTIONS, {'vacc_report': [vp, vp, u32, u32, vp, vp]}, 'vacc_version', VACC_VERSION)


def group_sizes(age_start, table, nr_ages):
    """agents of every group (int64[MAX_GROUPS]) from the population's age_start and the per-age group table"""
    starts = np.asarray(age_start, dtype=np.int64).ravel()[:nr_ages + 1]
    return np.bincount(np.asarray(table[:nr_ages], dtype=np.int64), weights=np.diff(starts), minlength=MAX_GROUPS).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the specification

def report_numpy(hot, vacc_day, log, age_start, age_group, n_days):
    """The report of one state and its log (the specification of reina_vacc_report).  hot: uint32[N]; vacc_day: int32[N] (the
    cold record's field; looked at only where the hot word says VACCINATED); log: uint32[N] (txlog.py); age_start: first agent
    of each age ([A] = N, padded with N); age_group: group of each age (< MAX_GROUPS); n_days: the tables by day hold the days
    [0, n_days)."""
    hot = np.asarray(hot).view(np.uint32).ravel()
    n_days = check_n_days(n_days)
    log = np.asarray(log, dtype=np.uint32).ravel()
    table, n_groups, nr_ages, age_of = _rep.age_lookup(age_start, age_group)
    words = np.zeros(report_words(n_days), dtype=np.uint64)
    count = lambda cells, size: np.bincount(cells, minlength=size).astype(np.uint64)
    idx = np.flatnonzero((hot & (7 | H_VACCINATED)) != 0)
    w = hot[idx]
    st, sev = (w & 7).astype(np.int64), ((w >> 3) & 7).astype(np.int64)
    inf, vac = st != 0, (w & H_VACCINATED) != 0
    g = table[age_of(idx)].astype(np.int64)
    vd = np.where(vac, np.asarray(vacc_day).view(np.int32).ravel()[idx].astype(np.int64), -1)
    valid = vac & (vd >= 0) & (vd < _eng.MAX_DAYS)
    t = (log[idx] & 0xFFFF).astype(np.int64)
    tk = inf & (t < BEFORE)
    since = np.where(valid & tk, t - vd, 0)
    after = inf & valid & tk & (since < 0)
    status = np.where(~vac | after, UNVACCINATED, np.where(~valid | ~tk, UNDETERMINED, np.where(since <= PROTECTION_DAYS, RECENT, PROTECTED)))
    closed, dead, severe = st >= S_RECOVERED, st == S_DEAD, sev >= V_SEVERE
    cell = status * MAX_GROUPS + g
    words[SEVERITY:OUTCOME] = count((cell * SEVERITIES + sev)[inf], OUTCOME - SEVERITY)
    out = np.zeros((STATUSES * MAX_GROUPS, OUTCOME_FIELDS), dtype=np.uint64)
    for c, sel in enumerate((inf, inf & closed, inf & dead, inf & ((w & H_DETECTED) != 0))):
        out[:, c] = count(cell[sel], len(out))
    words[OUTCOME:SINCE] = out.ravel()
    timed = inf & ((status == RECENT) | (status == PROTECTED))
    sc = g * SINCE_BINS + np.clip(since, 0, SINCE_BINS - 1)
    half = MAX_GROUPS * SINCE_BINS
    words[SINCE:SINCE + half] = count(sc[timed], half)
    words[SINCE + half:POPULATION] = count(sc[timed & severe], half)
    pop = np.zeros((MAX_GROUPS, POPULATION_FIELDS), dtype=np.uint64)
    for c, sel in enumerate((vac, vac & ~inf, vac & inf)):
        pop[:, c] = count(g[sel], MAX_GROUPS)
    words[POPULATION:SCALARS] = pop.ravel()
    a, b, c = vaccinations_offset(n_days), infections_offset(n_days), cohort_offset(n_days)
    vin = valid & (vd < n_days)
    words[a:b] = count((vd * MAX_GROUPS + g)[vin], b - a)
    dated = inf & (status < DATED_STATUSES) & tk
    tin = dated & (t < n_days)
    words[b:c] = count(((t * MAX_GROUPS + g) * DATED_STATUSES + status)[tin], c - b)
    coh = np.zeros((n_days * DATED_STATUSES, COHORT_FIELDS), dtype=np.uint64)
    key = t * DATED_STATUSES + status
    for k, sel in enumerate((tin, tin & severe, tin & dead, tin & closed)):
        coh[:, k] = count(key[sel], len(coh))
    words[c:] = coh.ravel()
    scalars = dict(vaccinated=int(vac.sum()), infected=int(inf.sum()), vaccinated_infected=int((vac & inf).sum()),
                   after_infection=int(after.sum()), undetermined=int((inf & (status == UNDETERMINED)).sum()),
                   bad_vacc_day=int((vac & ~valid).sum()),
                   out_of_range=int((valid & (vd >= n_days)).sum()) + int((dated & (t >= n_days)).sum()))
    for k, name in enumerate(SCALAR_NAMES):
        words[SCALARS + k] = scalars[name]
    return VaccinationReport(words, n_days, n_groups, group_sizes=group_sizes(age_start, table, nr_ages))


# ------------------------------------------------------------------------------------------------ reports

Share = collections.namedtuple('Share', 'share count')
Protection = collections.namedtuple('Protection', 'protection protected_share protected_count unvaccinated_share unvaccinated_count')
DeathProtection = collections.namedtuple('DeathProtection', Protection._fields + ('protected_closed_share', 'unvaccinated_closed_share'))


def _ratio(a, b):
    """a / b, None when b is 0 (an empty class has no share: what presymptomatic_share and the interval means do)"""
    return int(a) / int(b) if int(b) else None


def _status(status):
    return STATUS_NAMES.index(status) if isinstance(status, str) else int(status)


class VaccinationReport(_rep.Report):
    """One report: the words of include/reina_vaccination.h as named arrays, plus what is derived from them.  group_sizes: the
    agents of every age group (coverage_frame needs them; the words do not hold them)."""
    SCALARS, SCALAR_NAMES, IDENTITY = SCALARS, SCALAR_NAMES, ('n_days',)

    def __init__(self, words, n_days, n_groups=MAX_GROUPS, group_labels=None, start_date=None, group_sizes=None):
        self.n_days = n_days = int(n_days)
        w = self._take(words, report_words(n_days), 'a vaccination report of %d days has %d words' % (n_days, report_words(n_days)),
                       n_groups, group_labels)
        self.start_date = start_date
        self.group_sizes = None if group_sizes is None else np.asarray(group_sizes, dtype=np.int64)
        self.severity = w[SEVERITY:OUTCOME].reshape(STATUSES, MAX_GROUPS, SEVERITIES)
        self.outcome = w[OUTCOME:SINCE].reshape(STATUSES, MAX_GROUPS, OUTCOME_FIELDS)
        self.since = w[SINCE:POPULATION].reshape(SINCE_KINDS, MAX_GROUPS, SINCE_BINS)
        self.population = w[POPULATION:SCALARS].reshape(MAX_GROUPS, POPULATION_FIELDS)
        a, b, c = vaccinations_offset(n_days), infections_offset(n_days), cohort_offset(n_days)
        self.vaccinations = w[a:b].reshape(n_days, MAX_GROUPS)
        self.infections = w[b:c].reshape(n_days, MAX_GROUPS, DATED_STATUSES)
        self.cohort = w[c:].reshape(n_days, DATED_STATUSES, COHORT_FIELDS)

    def __repr__(self):
        return 'VaccinationReport(days=%d, vaccinated=%d, infected=%d, breakthroughs=%d+%d, undetermined=%d)' % (
            self.n_days, self.vaccinated, self.infected, int(self.outcome[RECENT, :, 0].sum()), int(self.outcome[PROTECTED, :, 0].sum()),
            self.undetermined)

    def _frame(self, table):
        import pandas as pd
        return pd.DataFrame(table[:, :self.n_groups].astype(np.int64), index=self._dates(), columns=pd.Index(self._groups(), name='age_group'))

    def doses_frame(self):
        """vaccinations by date (rows) and age group (columns)"""
        return self._frame(self.vaccinations)

    def coverage_frame(self):
        """by date and age group: the share of the group vaccinated by the end of that day (cumulative doses / group size; NaN
        for an empty group)"""
        if self.group_sizes is None:
            raise ValueError('coverage_frame: this report was built without group sizes')
        f = self.doses_frame().cumsum()
        with np.errstate(divide='ignore', invalid='ignore'):
            return f / self.group_sizes[:self.n_groups].astype(np.float64)

    def infections_frame(self, status=None):
        """dated infections by date of infection and age group: of one status at infection (0..2 or its name), or of all three"""
        m = self.infections.sum(axis=2, dtype=np.uint64) if status is None else self.infections[:, :, self._dated(status)]
        return self._frame(m)

    @staticmethod
    def _dated(status):
        s = _status(status)
        if not 0 <= s < DATED_STATUSES:
            raise ValueError('the tables by day hold the statuses %s' % ', '.join(STATUS_NAMES[:DATED_STATUSES]))
        return s

    def breakthrough_share(self):
        """by date of infection: infections of vaccinated agents (recent + protected) over all dated infections (NaN on a day
        without one)"""
        import pandas as pd
        by = self.infections.sum(axis=1, dtype=np.uint64).astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            share = (by[:, RECENT] + by[:, PROTECTED]) / by.sum(axis=1)
        return pd.Series(share, index=self._dates(), name='breakthrough_share')

    def _by_group(self, table, group):
        """[status, ...] of a [status, group, ...] table: one group's, or summed over the groups"""
        return table.sum(axis=1, dtype=np.uint64) if group is None else table[:, int(group)]

    def severity_frame(self, group=None):
        """infected agents by status at infection (rows) and severity (columns), of one age group or of all"""
        import pandas as pd
        return pd.DataFrame(self._by_group(self.severity, group).astype(np.int64), index=pd.Index(STATUS_NAMES, name='status'),
                            columns=pd.Index(SEVERITY_NAMES, name='severity'))

    def outcome_frame(self, group=None):
        """infected agents by status at infection (rows): agents, closed, dead, detected"""
        import pandas as pd
        return pd.DataFrame(self._by_group(self.outcome, group).astype(np.int64), index=pd.Index(STATUS_NAMES, name='status'),
                            columns=list(OUTCOME_NAMES))

    def population_frame(self):
        """vaccinated agents by age group (rows): all, still susceptible, infected"""
        import pandas as pd
        return pd.DataFrame(self.population[:self.n_groups].astype(np.int64), index=pd.Index(self._groups(), name='age_group'),
                            columns=list(POPULATION_NAMES))

    def severe_share(self, status, group=None):
        """Share(share, count): the share of the agents infected with `status` whose severity is severe or worse (None when
        there are none) and their number.  Severity is drawn at infection: open cohorts are not censored for it."""
        s = self._by_group(self.severity, group)[_status(status)]
        n = int(s.sum())
        return Share(_ratio(s[V_SEVERE:].sum(), n), n)

    def protection_against_severe(self, group=None):
        """Protection: 1 - severe_share(protected) / severe_share(unvaccinated), with both shares and both counts.  None when a
        class is empty or no unvaccinated agent is severe."""
        p, u = self.severe_share(PROTECTED, group), self.severe_share(UNVACCINATED, group)
        value = 1.0 - p.share / u.share if p.share is not None and u.share else None
        return Protection(value, p.share, p.count, u.share, u.count)

    def protection_against_death(self, group=None):
        """DeathProtection: the same over the CLOSED agents only (dead / closed: an open case has no outcome yet), the counts
        being the closed agents, with the closed share of either class beside it"""
        o = self._by_group(self.outcome, group)
        (pn, pc, pd_), (un, uc, ud) = [[int(x) for x in o[s, :3]] for s in (PROTECTED, UNVACCINATED)]
        ps, us = _ratio(pd_, pc), _ratio(ud, uc)
        value = 1.0 - ps / us if ps is not None and us else None
        return DeathProtection(value, ps, pc, us, uc, _ratio(pc, pn), _ratio(uc, un))

    def since_vaccination(self, severe=False, group=None):
        """days from the dose to the infection of the agents infected after it (recent and protected), as txlog's interval
        object -- counts by value, series(), quantile(), mean(); the last bin holds the clipped values.  severe: those with a
        severity of severe or worse only.  The factor 0.1 shows as the step behind day 14 in the ratio of the two."""
        k = 1 if severe else 0
        counts = self.since[k].sum(axis=0, dtype=np.uint64) if group is None else self.since[k, int(group)]
        return _txl._Intervals(counts, 0, 'days_since_vaccination')

    def protection_by_cohort(self):
        """by date of infection, per status at infection (0..2): agents, severe, dead, closed -- columns (status, field)"""
        import pandas as pd
        cols = pd.MultiIndex.from_product([STATUS_NAMES[:DATED_STATUSES], COHORT_NAMES], names=['status', 'field'])
        return pd.DataFrame(self.cohort.reshape(self.n_days, -1).astype(np.int64), index=self._dates(), columns=cols)


# ------------------------------------------------------------------------------------------------ routes

def _sizes(ctx, table):
    return group_sizes(ctx.age_start, _group_table(table, ctx.nr_ages)[0], ctx.nr_ages)


VACCINATION = _rep.Kind(
    name='vaccination_reports', of='transmission_log', arguments=_txl.day_arguments, report=VaccinationReport, words=report_words,
    numpy=lambda ctx, tlog, table, params: lambda depth: report_numpy(
        _rep.host_state(ctx.engine)[0], _txl._host_array(ctx.engine.tensors['vacc_day']), tlog.words(), ctx.age_start, table, *params).words,
    names=('vacc_report', 'vacc_report'), entry=('vacc_f', 'vaccination-report', 'reina_vaccination.h'),
    extra=lambda ctx, table: (_sizes(ctx, table),))


def device_report_words(device_log, table, n_groups, n_days):
    """[members, report_words(n_days)] uint64 of a txlog.DeviceLog: one launch for all members"""
    return _rep.device_take(VACCINATION, device_log, table, n_groups, (n_days,))()


def report_log(tlog, age_groups=None, n_days=None):
    """TransmissionLog.vaccination_report (reports.report_of)"""
    return _rep.report_of(VACCINATION, tlog, age_groups, n_days)


def report_group(device_log, contexts, age_groups=None, n_days=None):
    """The reports of every member of a logged group (or of the one engine of a device log): one launch for all members."""
    return _rep.reports_of_device(VACCINATION, device_log, contexts, age_groups, n_days)
