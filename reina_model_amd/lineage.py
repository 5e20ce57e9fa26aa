"""Lineage reports: who infects whom by period, and the trees of a run by the period they were seeded in
(include/reina_lineage.h).

The engine knows who infected whom (transmission.py: every agent's tree); the transmission log knows when (txlog.py: every
agent's day of infection).  A lineage report, taken between two days of a log and the engine state it belongs to, joins the
two as exact integer counts.

  parameters    period_days in 1..4096; n_periods = P in 1..256, Q = P + 1; the age -> group table of the other reports
                (< 16 groups); max_depth as in transmission.report_numpy.
  period class  of a log half word d:  pc(d) = d // period_days when d is known (neither NONE nor BEFORE) and that quotient
                is < P; otherwise pc(d) = P (before the log, undated or out of range).

"Infected", "root", "link", "bad link", "converged" and "tree" are those of transmission.py: a bad link's agent heads a tree of
its own; agents whose root is not reached in the rounds run are unconverged and count in no tree.  t(.) is the log's infection
half word; an agent is alive in the states INCUBATION .. IN_ICU.  With i an infected agent, s its infector on a link and r the
root of a converged agent:

  scalars[16]          infected, links, bad_links, roots (infector -1), trees (roots plus bad-link heads), unconverged, rounds,
                       alive_agents (converged and alive), alive_trees, largest_tree, largest_root (smallest index on ties),
                       undated (infected agents with pc(t) = P)
  seed[Q][4]           by seed class pc(t(r)): trees, alive trees, converged agents, alive converged agents
  tree_sizes[Q][33]    trees by (seed class, floor(log2(size)))
  cohort[Q][16][2]     infected agents by (pc(t(i)), own age group): agents, those in a state >= RECOVERED
  lineage[Q][Q]        converged agents by (seed class of their root, pc(t(i)))
  mixing_t[Q][16][16]  links by (pc(t(i)), group of s, group of i): who infects whom by time of transmission
  mixing_c[Q][16][16]  links by (pc(t(s)), group of s, group of i): the next-generation counts of the cohort infected then

`report_numpy` is the executable specification: the library's kernels (k_lineage_links, k_tx_jump, k_lineage_tally,
k_lineage_roots) compute the same words.  It is also the path of logs kept in host memory.
"""
import ctypes

import numpy as np

from . import engine as _eng
from . import reports as _rep
from . import transmission as _tx  # noqa: F401  (rounds_for is read as lineage._tx.rounds_for)
from . import txlog as _txl

LINEAGE_VERSION = 1            # include/reina_lineage.h: REINA_LINEAGE_VERSION
MAX_PERIODS, MAX_GROUPS, SIZE_BINS, SEED_FIELDS, COHORT_FIELDS = 256, 16, 33, 4, 2
SCALARS = 0
SCALAR_NAMES = ('infected', 'links', 'bad_links', 'roots', 'trees', 'unconverged', 'rounds', 'alive_agents', 'alive_trees',
                'largest_tree', 'largest_root', 'undated', 'largest_key')
S_NR = 16
S_INCUBATION, S_IN_ICU, S_RECOVERED = 1, 4, 5   # csrc/reina_prims.h: RS_INCUBATION, RS_IN_ICU, RS_RECOVERED

LINEAGE_FUNCTIONS = ('lineage_version', 'lineage_report', 'group_lineage_report')


def seed_offset(P):
    return S_NR


def tree_sizes_offset(P):
    return seed_offset(P) + (int(P) + 1) * SEED_FIELDS


def cohort_offset(P):
    return tree_sizes_offset(P) + (int(P) + 1) * SIZE_BINS


def lineage_offset(P):
    return cohort_offset(P) + (int(P) + 1) * MAX_GROUPS * COHORT_FIELDS


def mixing_t_offset(P):
    return lineage_offset(P) + (int(P) + 1) ** 2


def mixing_c_offset(P):
    return mixing_t_offset(P) + (int(P) + 1) * MAX_GROUPS * MAX_GROUPS


def report_words(P):
    """include/reina_lineage.h: REINA_LINEAGE_REPORT_WORDS"""
    return mixing_c_offset(P) + (int(P) + 1) * MAX_GROUPS * MAX_GROUPS


def scratch_bytes(n_agents):
    """include/reina_lineage.h: REINA_LINEAGE_SCRATCH_BYTES"""
    return (int(n_agents) * 24 + 255) & ~255


def bind_lineage_abi(lib, prefix):
    """The lineage-report entry points of a library, or None when it has none."""
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    args = [vp, vp, u32, u32, u32, u32, vp, vp, vp]
    return _eng.bind_optional_abi(lib, prefix, LINEAGE_FUNCTIONS, {'lineage_report': args, 'group_lineage_report': args},
                                  'lineage_version', LINEAGE_VERSION)


def default_periods(day, period_days):
    """ceil(max(day, 1) / period_days): the periods that hold every day run so far"""
    return -(-max(int(day), 1) // int(period_days))


def check_periods(period_days, n_periods, day=None):
    """(period_days, n_periods) as integers in their ranges: the one statement of them, which every route takes before it
    builds or launches anything.  n_periods None: default_periods(day, period_days)"""
    period_days = int(period_days)
    if not 1 <= period_days <= _eng.MAX_DAYS:
        raise ValueError('period must be in [1, %d] days' % _eng.MAX_DAYS)
    n_periods = default_periods(day, period_days) if n_periods is None else int(n_periods)
    if not 1 <= n_periods <= MAX_PERIODS:
        raise ValueError('n_periods = %d: a lineage report holds 1 .. %d periods (take a longer period)' % (n_periods, MAX_PERIODS))
    return period_days, n_periods


def period_class(half, period_days, n_periods):
    """pc(.) of an array of log half words"""
    h = np.asarray(half).astype(np.int64)
    q = h // int(period_days)
    return np.where((h < _txl.BEFORE) & (q < n_periods), q, n_periods)


# ------------------------------------------------------------------------------------------------ the specification

def report_numpy(hot, infector, n_infected, log, age_start, age_group, period_days, n_periods, max_depth=None):
    """The report of one state and its log (the specification of reina_lineage_report).  hot: uint32[N]; infector, n_infected:
    int32[N] (the cold record's fields; n_infected is not read); log: uint32[N]; age_start: first agent of each age ([A] = N,
    padded with N); age_group: group of each age (< MAX_GROUPS); max_depth: the deepest generation resolved (None: N, which
    every chain without a cycle fits)."""
    hot = np.asarray(hot).view(np.uint32).ravel()
    n = len(hot)
    period_days, P = check_periods(period_days, n_periods)
    Q = P + 1
    log = np.asarray(log, dtype=np.uint32).ravel()
    table, n_groups, _, ages = _rep.age_lookup(age_start, age_group)
    rounds = _rep.rounds_for(n if max_depth is None else max_depth)
    words = np.zeros(report_words(P), dtype=np.uint64)

    state, idx, s, root, linked, bad = _rep.links(hot, infector)
    st = state[idx].astype(np.int64)
    pc = period_class(log & 0xFFFF, period_days, P)      # of every agent
    ci = pc[idx]
    g = table[ages(idx)].astype(np.int64)

    a, b = cohort_offset(P), lineage_offset(P)
    coh = np.zeros((Q * MAX_GROUPS, COHORT_FIELDS), dtype=np.uint64)
    coh[:, 0] = np.bincount(ci * MAX_GROUPS + g, minlength=len(coh))
    coh[:, 1] = np.bincount((ci * MAX_GROUPS + g)[st >= S_RECOVERED], minlength=len(coh))
    words[a:b] = coh.ravel()
    sl = s[linked]
    cell = table[ages(sl)].astype(np.int64) * MAX_GROUPS + g[linked]
    a, b, c = mixing_t_offset(P), mixing_c_offset(P), report_words(P)
    words[a:b] = np.bincount(ci[linked] * MAX_GROUPS * MAX_GROUPS + cell, minlength=b - a).astype(np.uint64)
    words[b:c] = np.bincount(pc[sl] * MAX_GROUPS * MAX_GROUPS + cell, minlength=c - b).astype(np.uint64)

    # the trees: pointer jumping as k_tx_jump runs it
    r, _, conv = _rep.forest(n, idx, s, linked, rounds)
    r = r[conv]                                          # the root of every converged agent
    alive = ((st >= S_INCUBATION) & (st <= S_IN_ICU))[conv]
    sc = pc[r]
    a, b = lineage_offset(P), mixing_t_offset(P)
    words[a:b] = np.bincount(sc * Q + ci[conv], minlength=b - a).astype(np.uint64)
    size = np.bincount(r, minlength=n)
    size_alive = np.bincount(r[alive], minlength=n)
    heads = np.flatnonzero(size)
    hs, hc = size[heads].astype(np.int64), pc[heads]
    seed = np.zeros((Q, SEED_FIELDS), dtype=np.uint64)
    seed[:, 0] = np.bincount(hc, minlength=Q)
    seed[:, 1] = np.bincount(hc[size_alive[heads] > 0], minlength=Q)
    seed[:, 2] = np.bincount(sc, minlength=Q)
    seed[:, 3] = np.bincount(sc[alive], minlength=Q)
    a, b, c = seed_offset(P), tree_sizes_offset(P), cohort_offset(P)
    words[a:b] = seed.ravel()
    bins = np.array([int(x).bit_length() - 1 for x in hs], dtype=np.int64)
    words[b:c] = np.bincount(hc * SIZE_BINS + bins, minlength=c - b).astype(np.uint64)
    val = dict(infected=len(idx), links=int(linked.sum()), bad_links=int(bad.sum()), roots=int(root.sum()), trees=len(heads),
               unconverged=int((~conv).sum()), rounds=rounds, alive_agents=int(alive.sum()),
               alive_trees=int((size_alive[heads] > 0).sum()), undated=int((ci == P).sum()))
    val['largest_tree'], val['largest_root'], val['largest_key'] = _rep.largest(heads, hs)
    for k, name in enumerate(SCALAR_NAMES):
        words[SCALARS + k] = val[name]
    return LineageReport(words, period_days, P, n_groups)


# ------------------------------------------------------------------------------------------------ reports

class LineageReport(_rep.Report):
    """One report: the words of include/reina_lineage.h as named arrays, plus what is derived from them on the host."""
    SCALARS, SCALAR_NAMES, IDENTITY = SCALARS, SCALAR_NAMES, ('period_days', 'n_periods')

    def __init__(self, words, period_days, n_periods, n_groups=MAX_GROUPS, group_labels=None, start_date=None):
        self.period_days, self.n_periods = check_periods(period_days, n_periods)
        P = self.n_periods
        w = self._take(words, report_words(P), 'a lineage report of %d periods has %d words' % (P, report_words(P)), n_groups,
                       group_labels)
        Q = P + 1
        self.start_date = start_date
        o = [seed_offset(P), tree_sizes_offset(P), cohort_offset(P), lineage_offset(P), mixing_t_offset(P), mixing_c_offset(P),
             report_words(P)]
        self.seed = w[o[0]:o[1]].reshape(Q, SEED_FIELDS)
        self.tree_sizes = w[o[1]:o[2]].reshape(Q, SIZE_BINS)
        self.cohort = w[o[2]:o[3]].reshape(Q, MAX_GROUPS, COHORT_FIELDS)
        self.lineage = w[o[3]:o[4]].reshape(Q, Q)
        self.mixing_t = w[o[4]:o[5]].reshape(Q, MAX_GROUPS, MAX_GROUPS)
        self.mixing_c = w[o[5]:o[6]].reshape(Q, MAX_GROUPS, MAX_GROUPS)

    def __repr__(self):
        return 'LineageReport(periods=%d x %d d, infected=%d, trees=%d, alive_trees=%d, largest_tree=%d)' % (
            self.n_periods, self.period_days, self.infected, self.trees, self.alive_trees, self.largest_tree)

    def _periods(self, name, before=True):
        """the index of the P periods (their first day, or its date), with 'before' for class P"""
        import pandas as pd
        first = [k * self.period_days for k in range(self.n_periods)]
        if self.start_date is not None:
            d0 = pd.Timestamp(str(self.start_date))
            first = [(d0 + pd.Timedelta(days=k)).date().isoformat() for k in first]
        return pd.Index(first + (['before'] if before else []), name=name, dtype=object)

    def mixing_frame(self, period, by='transmission'):
        """links of one period by infector's age group (rows) and infectee's (columns): by='transmission' the links made in
        that period, by='cohort' the links made by the agents infected in it"""
        import pandas as pd
        if by not in ('transmission', 'cohort'):
            raise ValueError("by: 'transmission' or 'cohort'")
        m = (self.mixing_t if by == 'transmission' else self.mixing_c)[int(period), :self.n_groups, :self.n_groups].astype(np.int64)
        labels = self._groups()
        return pd.DataFrame(m, index=pd.Index(labels, name='infector'), columns=pd.Index(labels, name='infectee'))

    def next_generation_matrix(self, period):
        """float64[n_groups, n_groups]: the infections so far by an agent of the row's group, infected in `period`, among the
        column's group (mixing_c over the infector group's cohort size); NaN rows for an empty group"""
        g = self.n_groups
        m = self.mixing_c[int(period), :g, :g].astype(np.float64)
        size = self.cohort[int(period), :g, 0].astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            return m / size[:, None]

    def reproduction_number(self):
        """per period of infection: R (the dominant eigenvalue of the cohort's next-generation matrix over its non-empty
        groups; NaN for an empty cohort), the cohort's size and the share of it that is removed (R of an open cohort is
        censored, as LogReport.case_reproduction_number says)"""
        import pandas as pd
        rows = []
        for p in range(self.n_periods):
            size = self.cohort[p, :self.n_groups, 0].astype(np.int64)
            have = np.flatnonzero(size)
            if not len(have):
                rows.append((np.nan, 0, np.nan))
                continue
            k = self.next_generation_matrix(p)[np.ix_(have, have)]
            removed = int(self.cohort[p, :, 1].sum())
            rows.append((float(np.max(np.abs(np.linalg.eigvals(k)))), int(size.sum()), removed / int(size.sum())))
        return pd.DataFrame(rows, columns=['r', 'cohort', 'closed_share'], index=self._periods('period', before=False))

    def lineage_frame(self):
        """converged agents by the period their tree was seeded in (rows, plus 'before') and the period of their own infection
        (columns)"""
        import pandas as pd
        return pd.DataFrame(self.lineage.astype(np.int64), index=self._periods('seeded'), columns=self._periods('infected'))

    def lineage_share(self):
        """lineage_frame normalised by column: the share of each period's infections that descends from each seeding period
        (NaN for a period without infections)"""
        f = self.lineage_frame().astype(np.float64)
        total = f.sum(axis=0)
        return f / total.where(total > 0)

    def introductions(self):
        """per seeding period: trees, alive trees, agents, alive agents, and the share of the trees that are extinct (NaN
        without trees)"""
        import pandas as pd
        s = self.seed.astype(np.int64)
        with np.errstate(divide='ignore', invalid='ignore'):
            extinct = 1.0 - s[:, 1] / s[:, 0].astype(np.float64)
        return pd.DataFrame(dict(trees=s[:, 0], alive_trees=s[:, 1], agents=s[:, 2], alive_agents=s[:, 3], extinct_share=extinct),
                            index=self._periods('seeded'))

    def tree_size_frame(self):
        """trees by seeding period (rows) and size class 2^b .. 2^(b+1) - 1 (columns, by their lower end)"""
        import pandas as pd
        return pd.DataFrame(self.tree_sizes.astype(np.int64), index=self._periods('seeded'),
                            columns=pd.Index([1 << b for b in range(SIZE_BINS)], name='size_from'))


# ------------------------------------------------------------------------------------------------ taking a report

_UNCONVERGED = SCALARS + SCALAR_NAMES.index('unconverged')


def _arguments(ctx, period, n_periods, age_groups):
    """(table, labels, period_days, n_periods) of a Context's route: its report groups, the periods checked (check_periods)"""
    table, labels = ctx._tx_groups(age_groups)
    return (table, labels) + check_periods(period, n_periods, ctx.day)


def _numpy(ctx, tlog, table, params):
    """report_numpy on host copies, read once for both passes.  Generations are resolved to the engine's day + 1 first; a state
    deeper than that (only a synthetic one can be) is reported again with every chain resolved (reports.with_deep_pass)."""
    hot, inf, cnt, counters = _rep.host_state(ctx.engine)
    log = tlog.words()
    return lambda depth: report_numpy(hot, inf, cnt, log, ctx.age_start, table, *params, depth or _rep.day_depth(counters)).words


LINEAGE = _rep.Kind(
    name='lineage_reports', of='transmission_log', arguments=_arguments, numpy=_numpy, report=LineageReport,
    words=lambda period_days, n_periods: report_words(n_periods), names=('lineage_report', 'group_lineage_report'),
    entry=('lineage_f', 'lineage-report', 'reina_lineage.h'), scratch=scratch_bytes, unconverged=_UNCONVERGED)


def report_log(tlog, period=7, n_periods=None, age_groups=None):
    """TransmissionLog.lineage_report (reports.report_of)"""
    return _rep.report_of(LINEAGE, tlog, period, n_periods, age_groups)


def report_group(device_log, contexts, period=7, n_periods=None, age_groups=None):
    """The reports of every member of a logged group (or of the one engine of a device log): one launch per pass for all
    members (and once more, with every chain resolved, when a member's first pass leaves agents unconverged)."""
    return _rep.reports_of_device(LINEAGE, device_log, contexts, period, n_periods, age_groups)
