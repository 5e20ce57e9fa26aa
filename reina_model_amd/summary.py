"""Ensemble summaries: quantile bands, sums, peaks and exceedance of the members' counter histories (include/reina_summary.h;
DESIGN.md section 6j).

An ensemble's history is [K, days, COUNTER_WORDS] int32 -- 341 MB for 128 members of a year -- and what is wanted of it is a few
hundred KB: per date the quantile band of every counter total and of every age group, per member the peak and its date, the
share of futures in which a series ever passes a capacity.  The summary is exact integer arithmetic:

  input    K members (1 .. 1024), each `days` rows (1 .. 4096) of COUNTER_WORDS int32; nr_ages in 1 .. 128; the age -> group
           table of the other reports, G <= 16 groups.
  series   every row is reduced to S = C_NR * (1 + G) + S_NR int32 values:
             c * (1 + G)              counter c summed over the ages [0, nr_ages)
             c * (1 + G) + 1 + g      the same sum over the ages whose group is g
             C_NR * (1 + G) + s       scalar slot s, copied
           words of ages >= nr_ages are ignored; the sums wrap as .sum(dtype=int32) does (no counter of a real run comes near
           it).  A quantile of a total is not a sum of quantiles, which is why the sums come first.
  report   int64 words, tables row-major:
             order[days][S][Q]     for Q <= 16 ranks 0 <= r_q <= K - 1: the r_q-th smallest of the K members' values
             sum[days][S]          the sum over the members
             peak[K][S][2]         each member's largest value over the days, and the first day on which it is reached
             final[K][S]           each member's value on the last day
             exceed[T][days]       for T <= 32 thresholds (series, value): the members whose series is > value on that day
             first_exceed[T][K]    each member's first such day, or -1
  ranks    from quantile levels by rank(q, K) = max(ceil(q * K) - 1, 0): the inverted CDF, the rule filtering.quantiles uses;
           for equal weights np.quantile(..., method='inverted_cdf').

`summarise_numpy` is the executable specification: the library's kernels (k_summary_series, k_summary_peak, k_summary_order)
compute the same words.  It is also the route of histories in host memory.

Out of scope: weighted quantiles (the particle filter's final weights), variances, the histories of sharded Contexts.
"""
import ctypes
import math

import numpy as np

from . import engine as _eng
from . import reports as _rep

SUMMARY_VERSION = 1            # include/reina_summary.h: REINA_SUMMARY_VERSION
MAX_MEMBERS, MAX_GROUPS, MAX_RANKS, MAX_THRESHOLDS, PEAK_FIELDS = 1024, 16, 16, 32, 2
SUMMARY_FUNCTIONS = ('summary_version', 'summary')
# the scalar slots a threshold or an accessor may name (include/reina_hip.h: REINA_S_*)
SCALAR_SLOTS = dict(available_beds=_eng.S_AVAILABLE_BEDS, available_icu=_eng.S_AVAILABLE_ICU, beds=_eng.S_BEDS,
                    icu_units=_eng.S_ICU_UNITS, total_infections=_eng.S_TOTAL_INFECTIONS, total_infectors=_eng.S_TOTAL_INFECTORS,
                    exposed_per_day=_eng.S_EXPOSED_PER_DAY, ct_cases_per_day=_eng.S_CT_CASES_PER_DAY, problem=_eng.S_PROBLEM,
                    day=_eng.S_DAY, unable_to_import=_eng.S_UNABLE_TO_IMPORT, queue_len=_eng.S_QUEUE_LEN)


class Threshold(ctypes.Structure):
    """reina_summary_threshold_t"""
    _fields_ = [('series', ctypes.c_uint32), ('value', ctypes.c_int32)]


def n_series(G):
    """include/reina_summary.h: REINA_SUMMARY_SERIES"""
    return _eng.C_NR * (1 + int(G)) + _eng.S_NR


def order_offset(K, days, S, Q, T):
    return 0


def sum_offset(K, days, S, Q, T):
    return order_offset(K, days, S, Q, T) + days * S * Q


def peak_offset(K, days, S, Q, T):
    return sum_offset(K, days, S, Q, T) + days * S


def final_offset(K, days, S, Q, T):
    return peak_offset(K, days, S, Q, T) + K * S * PEAK_FIELDS


def exceed_offset(K, days, S, Q, T):
    return final_offset(K, days, S, Q, T) + K * S


def first_exceed_offset(K, days, S, Q, T):
    return exceed_offset(K, days, S, Q, T) + T * days


def report_words(K, days, S, Q, T):
    """include/reina_summary.h: REINA_SUMMARY_REPORT_WORDS"""
    return first_exceed_offset(K, days, S, Q, T) + T * K


def head_bytes(K):
    """include/reina_summary.h: REINA_SUMMARY_HEAD_BYTES"""
    return (512 + int(K) * 8 + 255) & ~255


def scratch_bytes(K, days, S):
    """include/reina_summary.h: REINA_SUMMARY_SCRATCH_BYTES"""
    return head_bytes(K) + ((int(days) * int(K) * int(S) * 4 + 255) & ~255)


def bind_summary_abi(lib, prefix):
    """The summary entry points of a library, or None when it has none."""
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    return _eng.bind_optional_abi(lib, prefix, SUMMARY_FUNCTIONS,
                                  {'summary': [vp, u32, u32, u32, vp, u32, vp, u32, vp, u32, vp, vp, vp]},
                                  'summary_version', SUMMARY_VERSION)


def rank(q, K):
    """the rank of quantile level q among K equally weighted members: max(ceil(q * K) - 1, 0) (the inverted CDF)"""
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError('a quantile level is in [0, 1], not %r' % q)
    return max(int(math.ceil(q * int(K))) - 1, 0)


# ------------------------------------------------------------------------------------------------ what is asked for

class SummarySpec:
    """What a summary holds.  quantiles: levels in [0, 1], at most 16.  age_groups: None (a Context's report groups; the
    10-year bins of reports.default_age_groups where there is no Context), a dict(labels=, age_indices=) or the group of every
    age.  thresholds: (attr, value) or (attr, age_group_label, value), at most 32; attr is a POP_ATTRS (engine.C_NAMES) name
    or a scalar's (SCALAR_SLOTS)."""

    def __init__(self, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), age_groups=None, thresholds=()):
        self.quantiles = tuple(float(q) for q in quantiles)
        if len(self.quantiles) > MAX_RANKS:
            raise ValueError('a summary holds at most %d quantiles' % MAX_RANKS)
        for q in self.quantiles:
            rank(q, 1)
        self.age_groups = age_groups
        self.thresholds = tuple(tuple(t) for t in thresholds)
        if len(self.thresholds) > MAX_THRESHOLDS:
            raise ValueError('a summary holds at most %d thresholds' % MAX_THRESHOLDS)
        for t in self.thresholds:
            if len(t) not in (2, 3):
                raise ValueError('a threshold is (attr, value) or (attr, age_group_label, value), not %r' % (t,))
            series_base(t[0])
            if not -2 ** 31 <= int(t[-1]) < 2 ** 31:
                raise ValueError('a threshold value is an int32, not %r' % (t[-1],))

    def groups(self, nr_ages, ctx=None):
        """(uint8[MAX_AGES] table, G, labels) for a population of nr_ages ages"""
        ag = self.age_groups
        if ag is None and ctx is not None:
            g, labels = ctx._tx_groups(None)
        elif ag is None:
            g, labels = _rep.default_age_groups(nr_ages)
        elif isinstance(ag, dict):
            g, labels = np.asarray(ag['age_indices']), list(ag['labels'])
        else:
            g, labels = np.asarray(ag, dtype=np.int64), None
        table, G = _rep._group_table(g, nr_ages)
        if labels is None:
            labels = [str(k) for k in range(G)]
        G = max(G, len(labels))
        labels = list(labels) + [str(k) for k in range(len(labels), G)]
        if G > MAX_GROUPS:
            raise ValueError('age groups are 0 .. %d' % (MAX_GROUPS - 1))
        return table, G, [str(x) for x in labels]


def series_base(attr):
    """('counter', c) or ('scalar', slot) of a series name"""
    if attr in _eng.C_NAMES:
        return 'counter', _eng.C_NAMES.index(attr)
    if attr in SCALAR_SLOTS:
        return 'scalar', SCALAR_SLOTS[attr]
    raise ValueError('unknown attribute %r (have %s)' % (attr, ', '.join(_eng.C_NAMES + tuple(SCALAR_SLOTS))))


class Layout:
    """A spec resolved for K members, `days` days and a population: the group table, the ranks, the thresholds as (series,
    value) and the offsets of the block."""

    def __init__(self, spec, K, days, nr_ages, ctx=None):
        self.spec, self.K, self.days, self.nr_ages = spec, int(K), int(days), int(nr_ages)
        if not 1 <= self.K <= MAX_MEMBERS:
            raise ValueError('a summary is of 1 .. %d members, not %d' % (MAX_MEMBERS, self.K))
        if not 1 <= self.days <= _eng.MAX_DAYS:
            raise ValueError('a summary is of 1 .. %d days, not %d' % (_eng.MAX_DAYS, self.days))
        if not 1 <= self.nr_ages <= _eng.MAX_AGES:
            raise ValueError('nr_ages is in 1 .. %d, not %d' % (_eng.MAX_AGES, self.nr_ages))
        self.table, self.G, self.labels = spec.groups(self.nr_ages, ctx)
        self.S = n_series(self.G)
        self.ranks = np.array([rank(q, self.K) for q in spec.quantiles], dtype=np.uint32)
        self.Q, self.T = len(self.ranks), len(spec.thresholds)
        self.thresholds = [(self.series(t[0], t[1] if len(t) == 3 else None), int(t[-1])) for t in spec.thresholds]
        dims = (self.K, self.days, self.S, self.Q, self.T)
        self.offsets = [f(*dims) for f in (order_offset, sum_offset, peak_offset, final_offset, exceed_offset, first_exceed_offset,
                                           report_words)]
        self.words = self.offsets[-1]

    def series(self, attr, group=None):
        """the series of a counter's total (group None), of one of its age groups (by label), or of a scalar"""
        kind, k = series_base(attr)
        if kind == 'scalar':
            if group is not None:
                raise ValueError('%r is a scalar: it has no age groups' % attr)
            return _eng.C_NR * (1 + self.G) + k
        if group is None:
            return k * (1 + self.G)
        if str(group) not in self.labels:
            raise ValueError('unknown age group %r (have %s)' % (group, ', '.join(self.labels)))
        return k * (1 + self.G) + 1 + self.labels.index(str(group))


# ------------------------------------------------------------------------------------------------ the specification

def _host_history(history):
    """[K, days, COUNTER_WORDS] int32 of an array or a list of members' (or chunks') arrays"""
    if isinstance(history, (list, tuple)):
        parts = [np.asarray(h, dtype=np.int32) for h in history]
        history = np.concatenate([p[None] if p.ndim == 2 else p for p in parts])
    h = np.asarray(history, dtype=np.int32)
    if h.ndim != 3 or h.shape[2] != _eng.COUNTER_WORDS:
        raise ValueError('a history is [members, days, %d], not %s' % (_eng.COUNTER_WORDS, list(h.shape)))
    return h


def series_numpy(history, nr_ages, table, G):
    """int32[K, days, S]: the series of every row"""
    h = _host_history(history)
    K, days, A, C = h.shape[0], h.shape[1], _eng.MAX_AGES, _eng.C_NR
    per_age = h[:, :, :C * A].reshape(K, days, C, A)[..., :nr_ages]
    out = np.zeros((K, days, n_series(G)), dtype=np.int32)
    g_of = np.asarray(table)[:nr_ages]
    for c in range(C):
        out[:, :, c * (1 + G)] = per_age[:, :, c].sum(axis=-1, dtype=np.int32)
        for g in range(G):
            out[:, :, c * (1 + G) + 1 + g] = per_age[:, :, c][..., g_of == g].sum(axis=-1, dtype=np.int32)
    out[:, :, C * (1 + G):] = h[:, :, C * A:]
    return out


def summarise_numpy(history, nr_ages, spec, ctx=None):
    """The block's words, int64[report_words], of a history in host memory (the specification of reina_summary)."""
    h = _host_history(history)
    lay = Layout(spec, h.shape[0], h.shape[1], nr_ages, ctx)
    return _words_numpy(h, lay)


def _words_numpy(h, lay):
    K, days, S = lay.K, lay.days, lay.S
    ser = series_numpy(h, lay.nr_ages, lay.table, lay.G)
    w = np.zeros(lay.words, dtype=np.int64)
    o = lay.offsets
    w[o[0]:o[1]] = np.sort(ser, axis=0)[lay.ranks.astype(np.int64)].transpose(1, 2, 0).ravel()     # [Q, days, S] -> [days, S, Q]
    w[o[1]:o[2]] = ser.astype(np.int64).sum(axis=0).ravel()
    peak = np.zeros((K, S, PEAK_FIELDS), dtype=np.int64)
    peak[:, :, 0] = ser.max(axis=1)
    peak[:, :, 1] = ser.argmax(axis=1)                    # (the first day on which the largest value is reached)
    w[o[2]:o[3]] = peak.ravel()
    w[o[3]:o[4]] = ser[:, days - 1].ravel()
    for t, (s, value) in enumerate(lay.thresholds):
        above = ser[:, :, s] > value                      # [K, days]
        w[o[4] + t * days:o[4] + (t + 1) * days] = above.sum(axis=0)
        w[o[5] + t * K:o[5] + (t + 1) * K] = np.where(above.any(axis=1), above.argmax(axis=1), -1)
    return w


# ------------------------------------------------------------------------------------------------ the device route

_lib_f = None


def library():
    """the summary entry points of the HIP library (with its last_error), or None when it has none"""
    global _lib_f
    if _lib_f is None:
        lib = _eng.load_hip_library()
        f = bind_summary_abi(lib, 'reina_')
        if f is not None:
            f = dict(f)
            f['last_error'] = lib.reina_last_error
            f['last_error'].restype = ctypes.c_char_p
        _lib_f = (f,)
    return _lib_f[0]


def _device_members(history):
    """(the tensors kept alive, one device pointer per member, days) of a device tensor [K, days, COUNTER_WORDS] or a list of
    members' [days, COUNTER_WORDS] / chunks' [k, days, COUNTER_WORDS] tensors; None when `history` is not on a device"""
    parts = list(history) if isinstance(history, (list, tuple)) else [history]
    if not parts or not all(hasattr(p, 'data_ptr') and getattr(p, 'is_cuda', False) for p in parts):
        return None
    import torch
    keep, ptrs, days = [], [], None
    for p in parts:
        if p.dtype != torch.int32 or p.dim() not in (2, 3) or p.shape[-1] != _eng.COUNTER_WORDS:
            raise ValueError('a history is int32 [members, days, %d], not %s %s' % (_eng.COUNTER_WORDS, p.dtype, list(p.shape)))
        p = p.contiguous()
        k, d = (1, p.shape[0]) if p.dim() == 2 else (p.shape[0], p.shape[1])
        if days is not None and d != days:
            raise ValueError('the members of a summary have the same number of days (%d and %d)' % (days, d))
        days = d
        keep.append(p)
        ptrs += [p.data_ptr() + m * d * 4 * _eng.COUNTER_WORDS for m in range(k)]
    return keep, ptrs, days


def device_words(f, history_ptrs, lay, device, stream=None):
    """int64[report_words] of one reina_summary call on rows that are on `device` (a torch device): the launches are queued on
    the current stream, the block's read-back waits for them"""
    import torch
    scratch = torch.empty(scratch_bytes(lay.K, lay.days, lay.S), dtype=torch.uint8, device=device)
    rep = torch.empty(lay.words, dtype=torch.int64, device=device)
    bases = (ctypes.c_void_p * lay.K)(*[int(p) for p in history_ptrs])
    table = np.ascontiguousarray(lay.table, dtype=np.uint8)
    ranks = np.ascontiguousarray(lay.ranks, dtype=np.uint32)
    thr = (Threshold * max(lay.T, 1))(*[Threshold(s, v) for s, v in lay.thresholds])
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    rc = f['summary'](bases, lay.K, lay.days, lay.nr_ages, table.ctypes.data, lay.G, ranks.ctypes.data if lay.Q else None, lay.Q,
                      thr if lay.T else None, lay.T, scratch.data_ptr(), rep.data_ptr(), stream)
    if rc != 0:
        msg = f['last_error']()
        raise _eng.EngineError('summary failed (%d): %s' % (rc, msg.decode() if msg else ''))
    return rep.cpu().numpy()   # (the copy waits for the launches: the scratch may go)


def summarise(history, nr_ages, spec, ctx=None, start_date=None, start_day=0, members=None):
    """The EnsembleSummary of a history: by the library's kernels for a device tensor [K, days, COUNTER_WORDS] (or a list of
    members' or chunks' device tensors, which need not be contiguous) when the library has the entry points -- the rows are
    never read back --, by summarise_numpy otherwise.  ctx: a Context of the ensemble (its report groups and start date);
    members: a label per member (seeds)."""
    if ctx is not None and start_date is None:
        start_date = ctx.start_date
    dev = _device_members(history)
    f = library() if dev is not None else None
    if dev is not None and f is not None:
        keep, ptrs, days = dev
        lay = Layout(spec, len(ptrs), days, nr_ages, ctx)
        w = device_words(f, ptrs, lay, keep[0].device)
        del keep
    else:
        if dev is not None:   # (a library of the day ABI only)
            history = [p.cpu().numpy() for p in dev[0]]
        h = _host_history(history)
        lay = Layout(spec, h.shape[0], h.shape[1], nr_ages, ctx)
        w = _words_numpy(h, lay)
    return EnsembleSummary(w, lay, start_date, start_day, members)


class Pending:
    """The histories of an ensemble that runs in chunks (ensemble.run_ensemble(concurrent=...), simulation.run_monte_carlo),
    kept where they are -- device tensors of a device group -- until every chunk has run: finish() summarises all members in
    one call.  Holds the spec with its age groups resolved, not a Context: the chunks' engines may go."""

    def __init__(self, spec, ctx, start_day=0):
        self.nr_ages, self.start_date, self.start_day = ctx.nr_ages, ctx.start_date, int(start_day)
        table, _, labels = spec.groups(ctx.nr_ages, ctx)
        self.spec = SummarySpec(spec.quantiles, dict(labels=labels, age_indices=table[:ctx.nr_ages]), spec.thresholds)
        self.parts = []

    def add(self, rows):
        self.parts.append(rows)

    def finish(self, members=None):
        return summarise(self.parts, self.nr_ages, self.spec, start_date=self.start_date, start_day=self.start_day, members=members)


def of_group(summary, rows, contexts, start_day):
    """ensemble.run_group_plan's end with `summary`: a SummarySpec gives the group's EnsembleSummary; a Pending takes the rows
    and gives None"""
    if isinstance(summary, Pending):
        summary.add(rows)
        return None
    return summarise(rows, contexts[0].nr_ages, summary, ctx=contexts[0], start_day=start_day)


def check_group(summary, contexts, plan, record_history):
    """what run_group_plan refuses of a `summary` before anything runs"""
    if not isinstance(summary, (SummarySpec, Pending)):
        raise ValueError('summary: a summary.SummarySpec, not %r' % (summary,))
    if not record_history:
        raise ValueError('run_group_plan: a summary is of the recorded history (record_history=True)')
    spec = summary.spec if isinstance(summary, Pending) else summary
    Layout(spec, len(contexts), plan['days'], contexts[0].nr_ages, contexts[0])   # (raises on what a summary cannot hold)


# ------------------------------------------------------------------------------------------------ the result

class EnsembleSummary:
    """The block of one summary as named arrays (order, sum, peak, final, exceed, first_exceed), and frames of them."""

    def __init__(self, words, layout, start_date=None, start_day=0, members=None):
        w = np.asarray(words, dtype=np.int64).ravel()
        lay = self.layout = layout
        if len(w) != lay.words:
            raise ValueError('a summary of %d members, %d days, %d series, %d ranks and %d thresholds has %d words'
                             % (lay.K, lay.days, lay.S, lay.Q, lay.T, lay.words))
        self.words, self.spec = w, lay.spec
        self.n_members, self.days, self.quantiles = lay.K, lay.days, lay.spec.quantiles
        self.start_date, self.start_day = start_date, int(start_day)
        self.members = list(members) if members is not None else list(range(lay.K))
        if len(self.members) != lay.K:
            raise ValueError('one label per member')
        o, K, days, S, Q, T = lay.offsets, lay.K, lay.days, lay.S, lay.Q, lay.T
        self.order = w[o[0]:o[1]].reshape(days, S, Q)
        self.sum = w[o[1]:o[2]].reshape(days, S)
        self.peak = w[o[2]:o[3]].reshape(K, S, PEAK_FIELDS)
        self.final_values = w[o[3]:o[4]].reshape(K, S)
        self.exceed = w[o[4]:o[5]].reshape(T, days)
        self.first_exceed = w[o[5]:o[6]].reshape(T, K)

    def __repr__(self):
        return 'EnsembleSummary(members=%d, days=%d, groups=%d, quantiles=%s, thresholds=%d)' % (
            self.n_members, self.days, self.layout.G, list(self.quantiles), self.layout.T)

    def __eq__(self, other):
        return isinstance(other, EnsembleSummary) and np.array_equal(self.words, other.words) \
            and np.array_equal(self.layout.offsets, other.layout.offsets)

    def _date(self, day):
        from datetime import date, timedelta
        if self.start_date is None:
            return self.start_day + int(day)
        return date.fromisoformat(str(self.start_date)) + timedelta(days=self.start_day + int(day))

    def dates(self):
        """the date of every row (the day number where the summary has no start date)"""
        return [self._date(k) for k in range(self.days)]

    def _index(self):
        import pandas as pd
        return pd.Index(self.dates(), name='date')

    def band(self, attr, group=None):
        """by date, one column per quantile: the band of a counter's total, of one of its age groups or of a scalar"""
        import pandas as pd
        return pd.DataFrame(self.order[:, self.layout.series(attr, group), :], index=self._index(), columns=list(self.quantiles))

    def mean(self, attr, group=None):
        """by date: the mean over the members"""
        import pandas as pd
        return pd.Series(self.sum[:, self.layout.series(attr, group)] / float(self.n_members), index=self._index(), name=attr)

    def peaks(self, attr, group=None):
        """per member: the largest value and the first date on which it is reached"""
        import pandas as pd
        p = self.peak[:, self.layout.series(attr, group)]
        return pd.DataFrame(dict(value=p[:, 0], date=[self._date(d) for d in p[:, 1]]), index=pd.Index(self.members, name='member'))

    def final(self, attr, group=None):
        """per member: the value on the last day"""
        import pandas as pd
        return pd.Series(self.final_values[:, self.layout.series(attr, group)], index=pd.Index(self.members, name='member'), name=attr)

    def _threshold(self, attr, value, group=None):
        key = (self.layout.series(attr, group), int(value))
        if key not in self.layout.thresholds:
            raise ValueError('the summary was not asked for the threshold %s > %d (SummarySpec(thresholds=...))'
                             % (attr if group is None else '%s[%s]' % (attr, group), int(value)))
        return self.layout.thresholds.index(key)

    def exceedance(self, attr, value, group=None):
        """by date: the share of the members whose series is above `value`"""
        import pandas as pd
        return pd.Series(self.exceed[self._threshold(attr, value, group)] / float(self.n_members), index=self._index(), name=attr)

    def ever_exceeds(self, attr, value, group=None):
        """the share of the members whose series is above `value` on any day"""
        return float((self.first_exceed[self._threshold(attr, value, group)] >= 0).mean())

    def first_exceed_dates(self, attr, value, group=None):
        """per member: the first date on which its series is above `value`, None when it never is"""
        import pandas as pd
        first = self.first_exceed[self._threshold(attr, value, group)]
        return pd.Series([self._date(d) if d >= 0 else None for d in first], index=pd.Index(self.members, name='member'),
                         name=attr, dtype=object)

    def frame(self):
        """every counter total's band in one frame: by date, columns (attr, quantile)"""
        import pandas as pd
        cols = pd.MultiIndex.from_product([_eng.C_NAMES, list(self.quantiles)], names=['attr', 'quantile'])
        data = np.concatenate([self.order[:, self.layout.series(a), :] for a in _eng.C_NAMES], axis=1)
        return pd.DataFrame(data, index=self._index(), columns=cols)
