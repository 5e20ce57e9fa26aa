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
from . import transmission as _tx
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


def check_periods(period_days, n_periods):
    period_days, n_periods = int(period_days), int(n_periods)
    if not 1 <= period_days <= _eng.MAX_DAYS:
        raise ValueError('period_days must be in [1, %d]' % _eng.MAX_DAYS)
    if not 1 <= n_periods <= MAX_PERIODS:
        raise ValueError('n_periods must be in [1, %d]' % MAX_PERIODS)
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
    src = np.asarray(infector).view(np.int32).ravel().astype(np.int64)
    log = np.asarray(log, dtype=np.uint32).ravel()
    age_start = np.asarray(age_start, dtype=np.int64).ravel()
    nr_ages = min(len(np.asarray(age_group).ravel()), _eng.MAX_AGES, len(age_start) - 1)
    table, n_groups = _tx._group_table(age_group, nr_ages)
    max_depth = n if max_depth is None else int(max_depth)
    rounds = _tx.rounds_for(max_depth)
    words = np.zeros(report_words(P), dtype=np.uint64)

    # the links, as transmission.report_numpy and txlog.report_numpy classify them
    state = hot & 7
    idx = np.flatnonzero(state != 0)
    st = state[idx].astype(np.int64)
    s = src[idx]
    root = s == -1
    in_range = (s >= 0) & (s < n) & (s != idx)
    linked = np.zeros(len(idx), dtype=bool)
    linked[in_range] = state[s[in_range]] != 0
    bad = ~root & ~linked
    pc = period_class(log & 0xFFFF, period_days, P)      # of every agent
    ci = pc[idx]
    ages = lambda i: np.clip(np.searchsorted(age_start[:nr_ages + 1], i, side='right') - 1, 0, nr_ages - 1)
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
    parent = np.full(n, _tx._MARK, dtype=np.uint32)
    dist = np.zeros(n, dtype=np.uint32)
    parent[idx] = np.where(linked, s, idx).astype(np.uint32)
    dist[idx] = np.where(linked, 1, _tx._ROOTED).astype(np.uint32)
    parent, dist = _tx._jump(parent, dist, rounds)
    conv = (dist[idx] & _tx._ROOTED) != 0
    r = parent[idx][conv].astype(np.int64)               # the root of every converged agent
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
    if len(heads):
        big = int(hs.max())
        r0 = int(heads[hs == big][0])
        val.update(largest_tree=big, largest_root=r0, largest_key=big << 32 | (~r0 & 0xFFFFFFFF))
    else:
        val.update(largest_tree=0, largest_root=(1 << 64) - 1, largest_key=0)
    for k, name in enumerate(SCALAR_NAMES):
        words[SCALARS + k] = val[name]
    return LineageReport(words, period_days, P, n_groups)


# ------------------------------------------------------------------------------------------------ reports

class LineageReport:
    """One report: the words of include/reina_lineage.h as named arrays, plus what is derived from them on the host."""

    def __init__(self, words, period_days, n_periods, n_groups=MAX_GROUPS, group_labels=None, start_date=None):
        w = np.asarray(words, dtype=np.uint64).ravel()
        self.period_days, P = check_periods(period_days, n_periods)
        if len(w) != report_words(P):
            raise ValueError('a lineage report of %d periods has %d words' % (P, report_words(P)))
        Q = P + 1
        self.words, self.n_periods, self.n_groups = w, P, int(n_groups)
        self.group_labels = list(group_labels) if group_labels is not None else None
        self.start_date = start_date
        o = [seed_offset(P), tree_sizes_offset(P), cohort_offset(P), lineage_offset(P), mixing_t_offset(P), mixing_c_offset(P),
             report_words(P)]
        self.seed = w[o[0]:o[1]].reshape(Q, SEED_FIELDS)
        self.tree_sizes = w[o[1]:o[2]].reshape(Q, SIZE_BINS)
        self.cohort = w[o[2]:o[3]].reshape(Q, MAX_GROUPS, COHORT_FIELDS)
        self.lineage = w[o[3]:o[4]].reshape(Q, Q)
        self.mixing_t = w[o[4]:o[5]].reshape(Q, MAX_GROUPS, MAX_GROUPS)
        self.mixing_c = w[o[5]:o[6]].reshape(Q, MAX_GROUPS, MAX_GROUPS)
        for k, name in enumerate(SCALAR_NAMES):
            setattr(self, name, int(w[SCALARS + k]))
        if self.largest_root == (1 << 64) - 1:
            self.largest_root = -1

    def __eq__(self, other):
        return isinstance(other, LineageReport) and (self.period_days, self.n_periods) == (other.period_days, other.n_periods) \
            and np.array_equal(self.words, other.words)

    def __repr__(self):
        return 'LineageReport(periods=%d x %d d, infected=%d, trees=%d, alive_trees=%d, largest_tree=%d)' % (
            self.n_periods, self.period_days, self.infected, self.trees, self.alive_trees, self.largest_tree)

    def _groups(self):
        return self.group_labels or [str(k) for k in range(self.n_groups)]

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

def _lineage_f(engine):
    f = getattr(engine, 'lineage_f', None)
    if f is None:
        raise _eng.EngineError('the engine library has no lineage-report entry points (include/reina_lineage.h)')
    return f


def default_periods(day, period_days):
    """ceil(max(day, 1) / period_days): the periods that hold every day run so far"""
    return -(-max(int(day), 1) // int(period_days))


def device_words(device_log, table, n_groups, period_days, n_periods, max_depth):
    """[members, report_words(n_periods)] uint64 of a txlog.DeviceLog: one launch per pass for all members"""
    e = device_log.engine
    f = _lineage_f(e)
    torch, dev = e.alloc.torch, e.alloc.device
    K, n = device_log.members, e.config.n_agents
    scratch = [torch.empty(scratch_bytes(n), dtype=torch.uint8, device=dev) for _ in range(K)]
    rep = torch.empty(K * report_words(n_periods), dtype=torch.int64, device=dev)
    if device_log.group is None:
        e._check(f['lineage_report'](device_log._h, table.ctypes.data, int(n_groups), int(period_days), int(n_periods), int(max_depth),
                                     scratch[0].data_ptr(), rep.data_ptr(), e.alloc.stream()), 'lineage_report')
    else:
        ptrs = (ctypes.c_void_p * K)(*[s.data_ptr() for s in scratch])
        e._check(f['group_lineage_report'](device_log._h, table.ctypes.data, int(n_groups), int(period_days), int(n_periods),
                                           int(max_depth), ptrs, rep.data_ptr(), e.alloc.stream()), 'group_lineage_report')
    device_log._touch()
    words = rep.cpu().numpy().view(np.uint64).reshape(K, report_words(n_periods))
    del scratch
    return words


def _arguments(ctx, period, n_periods, age_groups):
    table, labels = ctx._tx_groups(age_groups)
    period = int(period)
    if not 1 <= period <= _eng.MAX_DAYS:
        raise ValueError('period must be in [1, %d] days' % _eng.MAX_DAYS)
    n_periods = default_periods(ctx.day, period) if n_periods is None else int(n_periods)
    if not 1 <= n_periods <= MAX_PERIODS:
        raise ValueError('n_periods = %d: a lineage report holds 1 .. %d periods (take a longer period)' % (n_periods, MAX_PERIODS))
    return table, labels, period, n_periods


_UNCONVERGED = SCALARS + SCALAR_NAMES.index('unconverged')


def report_log(tlog, period=7, n_periods=None, age_groups=None):
    """TransmissionLog.lineage_report: the library's kernels when it has the entry points and the log is a single engine's on
    the device, report_numpy on host copies otherwise.  Generations are resolved to the engine's day + 1 first; a state deeper
    than that (only a synthetic one can be) is reported again with every chain resolved."""
    ctx = tlog.ctx
    table, labels, period, P = _arguments(ctx, period, n_periods, age_groups)
    e = ctx.engine
    n = e.config.n_agents
    dlog = tlog.device
    if dlog is not None and dlog.group is None and getattr(e, 'lineage_f', None) is not None:
        t8, ng = _tx._group_table(table, ctx.nr_ages)
        ng = max(ng, len(labels))
        w = device_words(dlog, t8, ng, period, P, 0)[0]
        if w[_UNCONVERGED]:
            w = device_words(dlog, t8, ng, period, P, n)[0]
    else:
        host = _txl._host_array
        hot = host(e.tensors['hot'])
        cold = host(e.tensors['cold']).view(np.uint32).reshape(n, _eng.COLD_WORDS)
        args = (hot, cold[:, 2], cold[:, 3], tlog.words(), ctx.age_start, table, period, P)
        w = report_numpy(*args, _tx._day_depth(host(e.tensors['counters']))).words
        if w[_UNCONVERGED]:
            w = report_numpy(*args, n).words
    return LineageReport(w, period, P, len(labels), labels, ctx.start_date)


def report_group(device_log, contexts, period=7, n_periods=None, age_groups=None):
    """The reports of every member of a logged group: one launch per pass for all members (and once more, with every chain
    resolved, when a member's first pass leaves agents unconverged)."""
    c0 = contexts[0]
    table, labels, period, P = _arguments(c0, period, n_periods, age_groups)
    t8, ng = _tx._group_table(table, c0.nr_ages)
    ng = max(ng, len(labels))
    w = device_words(device_log, t8, ng, period, P, 0)
    deep = np.flatnonzero(w[:, _UNCONVERGED])
    if len(deep):
        w[deep] = device_words(device_log, t8, ng, period, P, c0.engine.config.n_agents)[deep]
    return [LineageReport(w[m].copy(), period, P, len(labels), labels, c.start_date) for m, c in enumerate(contexts)]
