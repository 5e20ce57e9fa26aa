"""Particle filters: condition a Monte-Carlo ensemble on observed case counts (include/reina_filter.h; DESIGN.md "Particle
filter").

A bootstrap particle filter (sequential Monte Carlo) over ONE engine group: K member Contexts of one scenario, differing
only in their seed, run window by window from one planner's plans (Context.make_plan + ensemble.run_group_plan).  After
each window the members' history rows are scored against the observations on the host (a negative-binomial observation
model, float64), the weights are updated and, when the effective sample size falls below ess_threshold * K, the members
are resampled systematically.  Resampling moves device state only: member dst is overwritten by member src's carried
state (reina_group_clone: one launch for all pairs) and continues as an independent future under its own seed -- the RNG
is Philox keyed by the seed, so nothing is reseeded, and under one plan the members' host state is the same.

A LOGGED filter (txlog=True / course=True; include/reina_filter_log.h, DESIGN.md section 6d "Logged filters") keeps the dated
transmission log and the clinical course log of the whole group, and every clone carries them: after it a particle's log is
the log of its whole ancestral path, so the reports of the final particles (FilterResult.log_reports, course_reports,
reproduction_number_band, ...) are conditioned on the observations with no stitching on the host.

This module also holds clone_state, the numpy specification of the clone and the path for host-memory engines, and
clone_log_numpy / clone_course_numpy / clone_log_delta_numpy, those of the logs' clone.

Alignment: an observation dated t is scored against history row d = t - start_date, the state before day d (what the
reference's frames show on that date).  Rows outside the filter's horizon are ignored.
"""
import ctypes
import math
import time
from datetime import date, datetime

import numpy as np

from . import engine as _eng
from . import reports as _rep

FILTER_VERSION = 1              # include/reina_filter.h: REINA_FILTER_VERSION
CLONE_MAX_PAIRS = 896           # REINA_CLONE_MAX_PAIRS: pairs per launch
FILTER_FUNCTIONS = ('filter_version', 'group_clone')
FILTER_LOG_VERSION = 1          # include/reina_filter_log.h: REINA_FILTER_LOG_VERSION
FILTER_LOG_FUNCTIONS = ('filter_log_version', 'group_txlog_clone')
TILE = 512
# k_init's cold record: claim (2 words) ~0, infector -1, n_infected 0, onset 0.0, vacc_day -1, first_infectee -1, next_sibling -1
COLD_DEFAULT = np.array([0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
L_QUEUE0 = 2                    # REINA_L_QUEUE0 (queue1, level1 follow)
# observed stream -> (counter, cumulative?): cumulative streams are compared as increments between observed dates
STREAMS = {'all_detected': ('all_detected', True), 'dead': ('dead', True),
           'in_ward': ('in_ward', False), 'in_icu': ('in_icu', False)}


def bind_filter_abi(lib, prefix):
    """The particle-filter entry points of a library, or None when it has none."""
    argtypes = {'group_clone': [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]}
    return _eng.bind_optional_abi(lib, prefix, FILTER_FUNCTIONS, argtypes, 'filter_version', FILTER_VERSION)


def bind_filter_log_abi(lib, prefix):
    """The logged clone's entry points of a library (include/reina_filter_log.h), or None when it has none."""
    argtypes = {'group_txlog_clone': [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]}
    return _eng.bind_optional_abi(lib, prefix, FILTER_LOG_FUNCTIONS, argtypes, 'filter_log_version', FILTER_LOG_VERSION)


# ------------------------------------------------------------------------------------------------ the clone

def clone_state(dst, src, n_agents, max_queue):
    """The specification of reina_group_clone for one pair: dst (a dict of uint32 numpy arrays: hot [n], cold [n, 8],
    infectees [n, 8], counters, control, queue0, queue1, level1, active_bits, infected_bits) gets src's carried state, in
    place.  Agents recorded in src get src's hot word, cold record and slots; agents recorded only in dst get k_init's
    words; agents susceptible in both are not touched.  The bit-plane words of the n_tiles tiles, the dense blocks, and the
    queues up to src's lengths (clamped to [0, max_queue]) are copied."""
    n = int(n_agents)
    sh, dh = src['hot'][:n], dst['hot'][:n]
    rec = sh != 0
    clear = ~rec & (dh != 0)
    dst['cold'][rec] = src['cold'][rec]
    dst['infectees'][rec] = src['infectees'][rec]
    dst['cold'][clear] = COLD_DEFAULT
    dst['infectees'][clear] = 0xFFFFFFFF
    dh[:] = sh
    for name in ('counters', 'control'):
        dst[name][:] = src[name]
    for k, name in enumerate(('queue0', 'queue1', 'level1')):
        ln = min(max(int(np.int32(src['control'][L_QUEUE0 + k])), 0), int(max_queue))
        dst[name][:ln] = src[name][:ln]
    w = 16 * ((n + TILE - 1) // TILE)
    for name in ('active_bits', 'infected_bits'):
        dst[name][:w] = src[name][:w]


def _host_arrays(engine):
    """the carried arrays of a host-memory engine as writable uint32 views"""
    t = engine.tensors
    n = engine.config.n_agents
    v = lambda name: np.asarray(t[name]).view(np.uint32)
    out = {k: v(k) for k in ('hot', 'counters', 'control', 'queue0', 'queue1', 'level1', 'active_bits', 'infected_bits')}
    out['cold'] = v('cold').reshape(n, _eng.COLD_WORDS)
    out['infectees'] = v('infectees').reshape(n, _eng.INLINE_INFECTEES)
    return out


def check_pairs(pairs, K):
    """(dst, src) pairs as an int64 [n, 2] array; ValueError on what reina_group_clone refuses (but testing_ever)"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(p) and (p.min() < 0 or p.max() >= K):
        raise ValueError('clone: a member index is out of range')
    if len(np.unique(p[:, 0])) != len(p):
        raise ValueError('clone: a destination appears twice')
    if np.intersect1d(p[:, 0], p[:, 1]).size:
        raise ValueError('clone: a source is also a destination')
    return p


def clone_log_numpy(dst_words, src_words):
    """The specification of reina_group_txlog_clone for one pair's log words (uint32 [n]): a dense copy, in place."""
    dst_words[:] = src_words
    return dst_words


def clone_course_numpy(dst_records, src_records):
    """... and for one pair's course records (uint64 [n])"""
    dst_records[:] = src_records
    return dst_records


def clone_log_delta_numpy(dst, src, dst_hot, src_hot):
    """k_txlog_clone's rule, for log words and for course records alike, in place: an agent whose hot word is non-zero in
    either member gets src's word; agents susceptible in both are not touched.  Equal to the dense copy on the logs'
    invariant: hot == 0 => the log word is NONE | NONE << 16 and the record four NONE (the begin and record passes write only
    where the state is not 0, and a hot word never returns to 0)."""
    touched = (np.asarray(dst_hot).view(np.uint32).ravel() != 0) | (np.asarray(src_hot).view(np.uint32).ravel() != 0)
    dst[touched] = np.asarray(src)[touched]
    return dst


def _group_log(contexts, group):
    """The txlog.DeviceLog of a filter's members (reports.shared_log): None when none of them keeps a transmission log, the
    group's log when they are the whole of ONE logged group and that group is `group`.  A clone carries the log of its group
    only: members that keep logs of their own, or of another group, are refused."""
    return _rep.shared_log(contexts, group, 'particle filter: members that keep a transmission log of their own, or of another '
                           "group, are refused (a clone carries the log of the filter's own group only: particle_filter(..., "
                           'txlog=True))')


def clone_group(group, pairs, log=None):
    """Member dst of the engine group gets member src's carried state, for every (dst, src) in `pairs`: ONE launch on the
    device (reina_group_clone), clone_state per pair for host-memory engines.  `log` (the txlog.DeviceLog of this group):
    dst gets src's log words as well, and its course records when a course is attached -- one call
    (reina_group_txlog_clone: the log's launch ahead of the state's)."""
    engines = group.engines
    e0 = engines[0]
    if log is None and not _eng.is_device(e0):
        p = check_pairs(pairs, len(engines))
        mq = min(e.config.max_queue for e in engines)
        for d, s in p:
            clone_state(_host_arrays(engines[d]), _host_arrays(engines[s]), e0.config.n_agents, mq)
        return
    if log is not None:
        f = _rep.entry_points(e0, 'filter_log_f', 'logged-clone', 'reina_filter_log.h')
        if getattr(log, 'group', None) is not group:
            raise ValueError('clone: `log` is not the transmission log of this group')
        name, owner = 'group_txlog_clone', log
    else:
        f = getattr(e0, 'filter_f', None)
        if f is None:
            raise _eng.EngineError('the engine library has no particle-filter entry points (include/reina_filter.h)')
        name, owner = 'group_clone', group
    flat = [int(x) for pr in pairs for x in pr]
    if len(flat) % 2:
        raise ValueError('clone: pairs are (dst, src)')
    arr = (ctypes.c_uint32 * max(len(flat), 1))(*[x & 0xFFFFFFFF for x in flat])
    _eng.mark_stale(engines)
    e0._check(f[name](owner._h, arr, len(flat) // 2, e0.alloc.stream()), name)


# ------------------------------------------------------------------------------------------------ observation model

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def nb_logpmf(y, mu, r):
    """negative-binomial log-pmf of count y with mean mu and dispersion r (variance mu + mu^2 / r), float64:
    lgamma(y + r) - lgamma(r) - lgamma(y + 1) + r log(r / (r + mu)) + y log(mu / (r + mu))"""
    y = np.asarray(y, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    r = float(r)
    p = r / (r + mu)   # (log(mu / (r + mu)) as log1p(-p): the form scipy.stats.nbinom uses)
    return _lgamma(y + r) - _lgamma(y + 1.0) - math.lgamma(r) + r * np.log(p) + y * np.log1p(-p)


class ObservationModel:
    """Negative-binomial observation model: streams = {stream: dispersion r}, stream one of STREAMS.  A simulated value is
    the sum over ages of the stream's counter; its mean is max(value, floor).  Cumulative streams (all_detected, dead)
    compare increments between consecutive observed dates inside the horizon (a negative observed increment counts as 0),
    level streams (in_ward, in_icu) the level."""

    def __init__(self, streams=None, floor=0.5):
        streams = {'all_detected': 10.0} if streams is None else dict(streams)
        if not streams:
            raise ValueError('ObservationModel: no stream')
        for s, r in streams.items():
            if s not in STREAMS:
                raise ValueError('ObservationModel: unknown stream %r (have %s)' % (s, ', '.join(STREAMS)))
            if not (float(r) > 0 and math.isfinite(float(r))):
                raise ValueError('ObservationModel: the dispersion of %r must be positive' % s)
        if not float(floor) > 0:
            raise ValueError('ObservationModel: floor must be positive')
        self.streams = {s: float(r) for s, r in streams.items()}
        self.floor = float(floor)

    def logpmf(self, y, sim, stream):
        return nb_logpmf(y, np.maximum(np.asarray(sim, dtype=np.float64), self.floor), self.streams[stream])


def _as_date(x):
    if isinstance(x, datetime):
        return x.date()
    if isinstance(x, date):
        return x
    if hasattr(x, 'date') and callable(x.date):   # pandas Timestamp
        return x.date()
    return date.fromisoformat(str(x)[:10])


def align(observations, start_date, first_row, end_row, streams):
    """{stream: (rows int64[n], values float64[n])}: the observed dates of each stream as history rows (days since
    start_date), sorted, those in [first_row, end_row) only; missing values (NaN / None) skipped."""
    import pandas as pd
    df = observations if isinstance(observations, pd.DataFrame) else pd.DataFrame(observations)
    d0 = _as_date(start_date)
    out = {}
    for s in streams:
        if s not in df.columns:
            raise ValueError('observations have no column %r' % s)
        col = pd.to_numeric(df[s], errors='coerce')
        rows, vals = [], []
        for t, v in zip(df.index, col.to_numpy(dtype=np.float64)):
            if not math.isfinite(v):
                continue
            d = (_as_date(t) - d0).days
            if first_row <= d < end_row:
                rows.append(d)
                vals.append(v)
        rows = np.asarray(rows, dtype=np.int64)
        vals = np.asarray(vals, dtype=np.float64)
        order = np.argsort(rows, kind='stable')
        rows, vals = rows[order], vals[order]
        if len(rows) and np.any(np.diff(rows) == 0):
            raise ValueError('observations of %r list a date twice' % s)
        out[s] = (rows, vals)
    return out


class _Scorer:
    """Per-window log-likelihoods of the members from their history rows; carries, per cumulative stream, every member's
    simulated value at the last observed row of the windows before (permuted with the members at a resample)."""

    def __init__(self, model, aligned, K):
        self.model = model
        self.terms = {}
        for s, (rows, vals) in aligned.items():
            if STREAMS[s][1]:
                # (row, observed increment, previous observed row): a term per observed date after the first
                self.terms[s] = [(int(rows[j]), max(vals[j] - vals[j - 1], 0.0), int(rows[j - 1])) for j in range(1, len(rows))]
            else:
                self.terms[s] = [(int(rows[j]), float(vals[j]), None) for j in range(len(rows))]
        self.rows = {s: aligned[s][0] for s in aligned}
        self.last = {s: np.zeros(K, dtype=np.int64) for s in aligned if STREAMS[s][1]}

    def score(self, hist, w0):
        """log-likelihood [K] of the window of history rows [w0, w0 + hist.shape[1])"""
        K, n = hist.shape[0], hist.shape[1]
        ll = np.zeros(K, dtype=np.float64)
        A = _eng.MAX_AGES
        for s, terms in self.terms.items():
            ci = _eng.C_NAMES.index(STREAMS[s][0])
            sim = None
            for row, y, prev in terms:
                if not w0 <= row < w0 + n:
                    continue
                if sim is None:
                    sim = hist[:, :, ci * A:(ci + 1) * A].astype(np.int64).sum(axis=2)
                cur = sim[:, row - w0]
                if prev is not None:
                    cur = cur - (sim[:, prev - w0] if prev >= w0 else self.last[s])
                ll += self.model.logpmf(y, cur, s)
            if s in self.last:
                rows = self.rows[s]
                inside = rows[(rows >= w0) & (rows < w0 + n)]
                if len(inside):
                    if sim is None:
                        sim = hist[:, :, ci * A:(ci + 1) * A].astype(np.int64).sum(axis=2)
                    self.last[s] = sim[:, int(inside[-1]) - w0].copy()
        return ll

    def permute(self, ancestors):
        for s in self.last:
            self.last[s] = self.last[s][ancestors]


# ------------------------------------------------------------------------------------------------ resampling

def logsumexp(x):
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x)
    if not math.isfinite(m):
        return m
    return float(m + math.log(np.sum(np.exp(x - m))))


def normalized(logw):
    """the weights exp(logw) / sum"""
    logw = np.asarray(logw, dtype=np.float64)
    w = np.exp(logw - np.max(logw))
    return w / w.sum()


def ess(weights):
    w = np.asarray(weights, dtype=np.float64)
    return float(1.0 / np.sum(w * w))


def systematic_offspring(weights, u):
    """offspring counts [K] of systematic resampling with the uniform u in [0, 1): member i gets floor(K W_i) or
    ceil(K W_i) copies, K in all"""
    w = np.asarray(weights, dtype=np.float64)
    K = len(w)
    cs = np.cumsum(w / w.sum())
    cs[-1] = 1.0
    idx = np.searchsorted(cs, (float(u) + np.arange(K)) / K, side='right')
    return np.bincount(np.minimum(idx, K - 1), minlength=K)


def assign_in_place(counts):
    """(ancestors [K], pairs [(dst, src)]) of offspring counts: every member with >= 1 offspring keeps its own state, the
    surplus copies go, in ascending index order, to the members with none -- so no source is ever a destination and only
    the members that died are written."""
    counts = np.asarray(counts, dtype=np.int64)
    K = len(counts)
    anc = np.arange(K, dtype=np.int64)
    surplus = np.repeat(np.arange(K), np.maximum(counts - 1, 0))
    dead = np.flatnonzero(counts == 0)
    assert len(surplus) == len(dead)
    anc[dead] = surplus
    return anc, [(int(d), int(s)) for d, s in zip(dead, surplus)]


# ------------------------------------------------------------------------------------------------ the driver

class FilterResult:
    """What particle_filter returns: per window (start_day, days, loglik [K], ess, ancestors [K], resampled); log_evidence;
    the final weights; the planner and the member Contexts (their engine group stays open for forecast(); close()).
    Of a logged filter also the posterior over what the logs report: log_reports / lineage_reports / course_reports of the
    final particles, and the weighted bands of R_c, incidence and admissions by date."""

    def __init__(self, planner, contexts, group, start_day, start_date, filter_seed):
        self.planner = planner
        self.contexts = contexts
        _group_log(contexts, group)
        self.group = group
        self.start_day = start_day
        self.start_date = _as_date(start_date)
        self.filter_seed = filter_seed
        self.windows = []
        self.log_evidence = 0.0
        self.logw = np.zeros(len(contexts), dtype=np.float64)
        self.timings = []
        # a filter that learns disease parameters (particle_filter(..., parameters=space)): the space, the device handle, the
        # members' log theta (the filter's state) and theta [K, P] (what the engines hold)
        self.space = None
        self.device_parameters = None
        self.log_theta = None
        self.parameters = None

    @property
    def n_particles(self):
        return len(self.contexts)

    @property
    def weights(self):
        return normalized(self.logw)

    @property
    def loglik(self):
        return np.stack([w['loglik'] for w in self.windows])

    @property
    def ess(self):
        return np.array([w['ess'] for w in self.windows])

    @property
    def ancestors(self):
        return np.stack([w['ancestors'] for w in self.windows])

    @property
    def days(self):
        return sum(w['days'] for w in self.windows)

    def paths(self):
        """history [K, days, COUNTER_WORDS] of every final particle, traced back through the ancestors"""
        K = self.n_particles
        idx = np.arange(K)
        parts = []
        for w in reversed(self.windows):
            idx = w['ancestors'][idx]
            parts.append(w['history'][idx])
        if not parts:
            return np.zeros((K, 0, _eng.COUNTER_WORDS), dtype=np.int32)
        return np.concatenate(parts[::-1], axis=1)

    def totals(self, attr):
        """[K, days]: the sum over ages of a POP_ATTRS counter along every path"""
        from .model import POP_ATTRS
        if attr not in POP_ATTRS:
            raise ValueError('unknown attribute %r (have %s)' % (attr, ', '.join(POP_ATTRS)))
        ci = _eng.C_NAMES.index(attr)
        A = _eng.MAX_AGES
        return self.paths()[:, :, ci * A:(ci + 1) * A].astype(np.int64).sum(axis=2)

    def dates(self):
        from datetime import timedelta
        return [self.start_date + timedelta(days=self.start_day + k) for k in range(self.days)]

    def quantiles(self, attr, q=(0.05, 0.5, 0.95)):
        """per-date quantiles of a POP_ATTRS total over the final particles, weighted by the final weights (inverted CDF):
        a DataFrame indexed by date, one column per q"""
        import pandas as pd
        q = [float(x) for x in np.atleast_1d(q)]
        return pd.DataFrame(self.weighted_band(self.totals(attr).astype(np.float64), q), index=self.dates(), columns=q)

    def weighted_band(self, values, q=(0.05, 0.5, 0.95), weights=None):
        """[T, len(q)]: per column of `values` [K, T] (float64, one row per final particle) the quantiles under the final
        weights (or `weights` [K]), by the inverted CDF -- the smallest value at which the cumulated weight reaches q.  Members
        whose value is not finite are left out of their column and the weights renormalised; a column with no finite value is NaN."""
        values = np.asarray(values, dtype=np.float64)
        if values.ndim != 2 or values.shape[0] != self.n_particles:
            raise ValueError('weighted_band: values are [n_particles, T]')
        w = self.weights if weights is None else np.asarray(weights, dtype=np.float64)
        q = [float(x) for x in np.atleast_1d(q)]
        out = np.full((values.shape[1], len(q)), np.nan)
        for d in range(values.shape[1]):
            keep = np.isfinite(values[:, d])
            if not keep.any():
                continue
            col, wk = values[keep, d], w[keep]
            order = np.argsort(col, kind='stable')
            v = col[order]
            cw = np.cumsum(wk[order])
            for j, x in enumerate(q):
                out[d, j] = v[min(int(np.searchsorted(cw, x * cw[-1] - 1e-12, side='left')), len(v) - 1)]
        return out

    def weighted_mean(self, values):
        """[T]: per column of `values` [K, T] the mean under the final weights, over the members whose value is finite (NaN
        when there is none)"""
        values = np.asarray(values, dtype=np.float64)
        keep = np.isfinite(values)
        w = self.weights[:, None] * keep
        tot = w.sum(axis=0)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(tot > 0, (np.where(keep, values, 0.0) * w).sum(axis=0) / tot, np.nan)

    # ---- a filter with parameters: the posterior over theta

    def _set_theta(self, log_theta):
        """the members' log theta: theta of it to all K device blocks by one call, and every Context's disease after it"""
        self.log_theta = np.asarray(log_theta, dtype=np.float64)
        self.parameters = self.space.theta_of(self.log_theta)
        dev = self.device_parameters
        dev.set(range(self.n_particles), self.parameters)
        for c, d in zip(self.contexts, dev.expand_many(self.parameters)):
            c._disease = d

    def _theta_windows(self, name):
        if self.space is None:
            raise ValueError('the filter learns no parameters (particle_filter(..., parameters=space))')
        p = self.space.index(name)
        from datetime import timedelta
        ws = [w for w in self.windows if w.get('theta') is not None]
        index = [self.start_date + timedelta(days=w['start_day'] + w['days'] - 1) for w in ws]
        return p, ws, index

    def parameter_band(self, name, q=(0.05, 0.5, 0.95)):
        """By window end date (the window's last day): the quantiles of knob `name` over the particles that ran the window,
        under that window's pre-resample weights (inverted CDF, weighted_band); a DataFrame, one column per q"""
        import pandas as pd
        p, ws, index = self._theta_windows(name)
        q = [float(x) for x in np.atleast_1d(q)]
        rows = [self.weighted_band(w['theta'][:, p:p + 1], q, weights=w['weights'])[0] for w in ws]
        return pd.DataFrame(np.asarray(rows).reshape(len(ws), len(q)), index=index, columns=q)

    def parameter_mean(self, name):
        """By window end date: the mean of knob `name` under the window's pre-resample weights (a Series)"""
        import pandas as pd
        p, ws, index = self._theta_windows(name)
        return pd.Series([float(np.sum(w['weights'] * w['theta'][:, p])) for w in ws], index=index, name=name)

    # ---- a logged filter: the posterior over the logs' reports

    @property
    def log(self):
        """the group's txlog.DeviceLog of a logged filter, None of an unlogged one"""
        return _group_log(self.contexts, self.group)

    def _reports(self, kind, *args):
        """the reports of one kind (reports.Kind) of every final particle (reports.reports_of_contexts)"""
        if self.group is None:
            raise ValueError('%s: the filter has been closed' % kind.name)
        glog = self.log
        if glog is None:
            raise ValueError('%s: the filter keeps no transmission log (particle_filter(..., txlog=True))' % kind.name)
        if kind.of == 'course_log' and glog.course is None:
            raise ValueError('%s: the filter keeps no course log (particle_filter(..., course=True))' % kind.name)
        return _rep.reports_of_contexts(kind, self.contexts, *args)

    def log_reports(self, age_groups=None, n_days=None):
        """txlog.LogReport of every final particle -- of its whole ancestral path -- by one launch (ensemble.log_reports)"""
        from .txlog import LOG
        return self._reports(LOG, age_groups, n_days)

    def lineage_reports(self, period=7, n_periods=None, age_groups=None):
        """lineage.LineageReport of every final particle, one launch per pass (ensemble.lineage_reports)"""
        from .lineage import LINEAGE
        return self._reports(LINEAGE, period, n_periods, age_groups)

    def course_reports(self, age_groups=None, n_days=None):
        """course.CourseReport of every final particle by one launch (ensemble.course_reports); needs course=True"""
        from .course import COURSE
        return self._reports(COURSE, age_groups, n_days)

    def vaccination_reports(self, age_groups=None, n_days=None):
        """vaccination.VaccinationReport of every final particle by one launch (ensemble.vaccination_reports): a clone carries
        the cold record, so a particle's days of vaccination are those of its whole ancestral path, like its log"""
        from .vaccination import VACCINATION
        return self._reports(VACCINATION, age_groups, n_days)

    def detection_reports(self, age_groups=None, n_days=None):
        """detection.DetectionReport of every final particle by one launch (ensemble.detection_reports); needs course=True.  A
        clone carries the cold records, the log and the course, so a particle's links and detections are its ancestral path's"""
        from .detection import DETECTION
        return self._reports(DETECTION, age_groups, n_days)

    def _band_frame(self, values, q, index, means=()):
        import pandas as pd
        q = [float(x) for x in np.atleast_1d(q)]
        df = pd.DataFrame(self.weighted_band(values, q), index=index, columns=q)
        for name, v in means:
            df[name] = self.weighted_mean(v)
        return df

    def reproduction_number_band(self, q=(0.05, 0.5, 0.95), variant=None):
        """By date of infection: the weighted quantiles over the final particles of the case reproduction number R_c
        (LogReport.case_reproduction_number; a particle whose cohort of the date is empty is left out of that date), one
        column per q, and the weighted means of the cohort's size (`cohort`) and of its closed share (`closed_share`: R_c of an
        open cohort is censored)."""
        frames = [r.case_reproduction_number(variant) for r in self.log_reports()]
        col = lambda name: np.stack([f[name].to_numpy(dtype=np.float64) for f in frames])
        return self._band_frame(col('r_c'), q, frames[0].index, (('cohort', col('cohort')), ('closed_share', col('closed_share'))))

    def incidence_band(self, q=(0.05, 0.5, 0.95)):
        """infections by date of infection, summed over variants and age groups: the weighted quantiles over the final particles"""
        reps = self.log_reports()
        return self._band_frame(np.stack([r.incidence.sum(axis=(1, 2), dtype=np.uint64).astype(np.float64) for r in reps]), q, reps[0]._dates())

    def admissions_band(self, q=(0.05, 0.5, 0.95)):
        """admissions by date, summed over age groups: the weighted quantiles over the final particles; needs course=True"""
        reps = self.course_reports()
        return self._band_frame(np.stack([r.admissions.sum(axis=1, dtype=np.uint64).astype(np.float64) for r in reps]), q, reps[0]._dates())

    def forecast(self, days):
        """continue the group `days` days with the planner's next plan, no observations (weights unchanged); returns
        history [K, days, COUNTER_WORDS]; paths() and quantiles() then extend over them.  A logged filter's logs are
        continued (its reports then reach the forecast's last day)"""
        from . import ensemble
        if self.group is None:
            raise ValueError('forecast: the filter has been closed')
        _group_log(self.contexts, self.group)
        d0 = self.start_day + self.days
        plan = self.planner.make_plan(int(days))
        hist = ensemble.run_group_plan(self.contexts, plan, group=self.group)
        K = self.n_particles
        self.windows.append(dict(start_day=d0, days=int(days), loglik=np.zeros(K), ess=ess(self.weights),
                                 ancestors=np.arange(K), resampled=False, history=hist, observed=False,
                                 theta=None if self.parameters is None else self.parameters.copy(), weights=self.weights))
        return hist

    def close(self):
        """closes the engine group -- the device parameters before it --, and a logged filter's log (and course) with it"""
        if self.device_parameters is not None:
            self.device_parameters.close()
            self.device_parameters = None
        if self.group is not None:
            try:
                glog = _group_log(self.contexts, self.group)
            except ValueError:
                glog = None
            if glog is not None:
                for c in self.contexts:
                    c.transmission_log = c.course_log = None
                glog.close()
            self.group.close()
            self.group = None


def particle_filter(variables, n_particles, observations=None, obs_model=None, window=7, days=None, seeds=None,
                    filter_seed=0, ess_threshold=0.5, device='cuda:0', engine_factory=None, age_counts=None, snapshot=None,
                    comm=None, txlog=False, course=False, parameters=None, shrinkage=0.98, policy=None):
    """Bootstrap particle filter of `n_particles` members of the scenario `variables` (seeds[m], default 0 .. K - 1) on
    `observations` (a DataFrame indexed by date, e.g. datasets.get_detected_cases; None: no observations, which is
    run_group_plan of the same seeds).  Windows of `window` days; after each one the members are scored with obs_model
    (default ObservationModel()) and resampled systematically (one uniform of numpy's PCG64(filter_seed) per resample) when
    the ESS < ess_threshold * K.  `days` (default: up to the last observed date, else variables['simulation_days']).
    `snapshot`: every member starts from that realised past (one group unpack, as ensemble.run_branches).
    `txlog`: the group keeps a dated transmission log (txlog.py), begun with the first window (with `snapshot`, the past is
    BEFORE), and every clone carries it (reina_group_txlog_clone); `course`: a clinical course log too (course.py; implies
    txlog).  The logs observe and never steer: histories, ancestors and evidence are those of the unlogged filter.  An engine
    library without the entry points raises EngineError.
    `parameters` (parameters.ParameterSpace): every particle carries a vector theta of multipliers on the disease block
    (include/reina_params.h).  theta is drawn from the knobs' priors at the start (after the snapshot's
    restore: the image is checked against the scenario's disease, the base), follows the particle's ancestor at every resample
    and is perturbed there by the Liu-West step with `shrinkage` (ParameterSpace.liu_west); between resamples it stays.  The
    initial population condition is applied when the members are made, BEFORE theta is set: its durations and severities are
    drawn under the scenario's own disease for every particle (ensemble.run_parameter_ensemble draws it under the member's
    theta).  One
    call (reina_group_params_set, queued behind the clone on the same stream) hands all K rows to the device.  Prior draws
    and perturbations come from a generator of their own, PCG64(SeedSequence([filter_seed, 1])): K x P draws at the start
    and at every resample; the resampling generator's draws are those of a filter without parameters.  log_evidence is then
    the evidence of scenario AND prior together.  The result's `parameters` is the final [K, P] table; parameter_band /
    parameter_mean give the posterior by window; windows[k] gains `theta` (in force during the window) and `weights` (its
    pre-resample weights).  An engine library without the entry points raises EngineError.
    Returns a FilterResult.  Sharded Contexts, K < 2, unknown streams and observations with no date inside the horizon are refused
    (ValueError; `comm`, a sharded population's communicator, and `policy`, a policy.Policy, are accepted only to be refused the
    same way); a failing
    member raises SimulationFailed."""
    from . import ensemble
    K = int(n_particles)
    if comm is not None:
        raise ValueError('particle_filter: sharded Contexts are not filtered')
    if policy is not None:
        raise ValueError('particle_filter: a policy is refused (a clone does not carry the policy state of its source)')
    if K < 2:
        raise ValueError('particle_filter: at least 2 particles')
    seeds = list(range(K)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != K:
        raise ValueError('particle_filter: one seed per particle')
    window = int(window)
    if window < 1:
        raise ValueError('particle_filter: window must be at least 1 day')
    if not 0.0 <= float(ess_threshold) <= 1.0:
        raise ValueError('particle_filter: ess_threshold is a share of K in [0, 1]')
    model = None
    if observations is not None:
        model = obs_model if obs_model is not None else ObservationModel()
        if not isinstance(model, ObservationModel):
            model = ObservationModel(dict(model))
    setup = ensemble.Setup(age_counts, device, engine_factory, None, None if snapshot is not None else 'auto', snapshot=snapshot)
    planner = setup.planner(variables, seeds[0])
    if planner.n_shards != 1 or planner.always_collective:
        raise ValueError('particle_filter: sharded Contexts are not filtered')
    txlog = bool(txlog or course)
    if txlog:
        _rep.entry_points(planner.engine, 'filter_log_f', 'logged-clone', 'reina_filter_log.h')
    if parameters is not None:
        _rep.entry_points(planner.engine, 'params_f', 'per-member parameter', 'reina_params.h')
        parameters.check(planner.nr_ages, planner.nr_variants)
        if not 0.5 < float(shrinkage) <= 1.0:
            raise ValueError('particle_filter: shrinkage is in (0.5, 1]')
    start_day = int(planner.day)
    if days is None:
        if observations is not None:
            al = align(observations, planner.start_date, start_day, 1 << 30, model.streams)
            last = max([int(r[-1]) for r, _ in al.values() if len(r)], default=start_day - 1)
            days = last + 1 - start_day
        else:
            days = int(variables['simulation_days']) - start_day
    days = int(days)
    if days < 1:
        raise ValueError('particle_filter: nothing to run (days = %d)' % days)
    scorer = None
    if observations is not None:
        aligned = align(observations, planner.start_date, start_day, start_day + days, model.streams)
        if not any(len(r) for r, _ in aligned.values()):
            raise ValueError('particle_filter: no observed date inside the horizon (days %d .. %d)' % (start_day, start_day + days - 1))
        scorer = _Scorer(model, aligned, K)
    ctxs = setup.members(variables, seeds)
    group, _ = ensemble.group_for(ctxs)
    res = FilterResult(planner, ctxs, group, start_day, planner.start_date, filter_seed)
    rng = np.random.Generator(np.random.PCG64(filter_seed))
    try:
        setup.restore_group(group, ctxs)
        if parameters is not None:
            from .parameters import DeviceParameters
            theta_rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(filter_seed), 1])))
            res.space = parameters
            res.device_parameters = DeviceParameters(group, planner._disease, parameters)
            res._set_theta(parameters.draw_prior(K, theta_rng))
        day = start_day
        while day < start_day + days:
            n = min(window, start_day + days - day)
            t0 = time.perf_counter()
            plan = planner.make_plan(n)
            hist = ensemble.run_group_plan(ctxs, plan, group=group, txlog=txlog, course=course)
            t1 = time.perf_counter()
            ll = scorer.score(hist, day) if scorer is not None else np.zeros(K)
            t2 = time.perf_counter()
            res.log_evidence += logsumexp(res.logw + ll) - logsumexp(res.logw)   # log sum_i W_i exp(ll_i)
            res.logw = res.logw + ll
            w = res.weights
            e = ess(w)
            anc, pairs, resampled = np.arange(K), [], False
            if e < float(ess_threshold) * K:
                anc, pairs = assign_in_place(systematic_offspring(w, rng.random()))
                res.logw = np.zeros(K)
                resampled = True
                if scorer is not None:
                    scorer.permute(anc)
            t3 = time.perf_counter()
            if pairs:
                clone_group(group, pairs, log=ctxs[0].transmission_log.device if txlog else None)
            t4 = time.perf_counter()
            theta = None if parameters is None else res.parameters.copy()   # (in force during this window)
            if parameters is not None and resampled:
                res._set_theta(parameters.liu_west(res.log_theta, w, anc, theta_rng.standard_normal((K, len(parameters))), shrinkage))
            t5 = time.perf_counter()
            res.windows.append(dict(start_day=day, days=n, loglik=ll, ess=e, ancestors=anc, resampled=resampled,
                                    history=hist, observed=scorer is not None, theta=theta, weights=w))
            res.timings.append(dict(run=t1 - t0, score=t2 - t1, resample=t3 - t2, clone=t4 - t3, pairs=len(pairs), params=t5 - t4))
            day += n
    except BaseException:
        res.close()
        raise
    return res
