"""A clinical course log: the day of detection, of admission, of ICU admission and of the outcome of every agent
(include/reina_course.h).

The transmission log (txlog.py) dates infection and onset.  A COURSE RECORD is one uint64 per agent, owned by the course log,
outside the engine state:

    record = detection_day | admission_day << 16 | icu_day << 32 | outcome_day << 48      codes: txlog.NONE, txlog.BEFORE

Days are absolute day numbers (Context.day, < 4096).  A field is KNOWN when it is neither code.  With w an agent's hot word,
st = w & 7 and DETECTED = w & 0x40:

  begin        st >= RECOVERED: all four fields BEFORE (the record is closed, its past unknown).  Otherwise detection BEFORE when
               st != 0 and DETECTED, admission BEFORE when st is HOSPITALIZED or IN_ICU, icu BEFORE when st is IN_ICU; every
               other field NONE.
  record day d with w the hot word after day d: nothing when the outcome is not NONE or st == 0.  Otherwise every field that is
               NONE gets d when its condition holds -- detection: DETECTED; admission: st is HOSPITALIZED or IN_ICU; icu: st is
               IN_ICU; outcome: st >= RECOVERED.  Nothing is ever overwritten, and a record CLOSES WITH ITS OUTCOME: a detection
               that reaches an agent later (contact tracing queues infectees whatever their state) is not dated and counts in
               the report's scalar detected_undated.
  report       between two days: detections, admissions, ICU admissions, deaths and recoveries by date and age group, the delay
               distributions between the dated events, the pathways through care, and the cohorts by date of infection behind
               the fatality and hospitalisation rates -- exact integer counts (CourseReport).

A course log is attached to a transmission log: it lives where the log lives (device or host memory), a report reads the
log's infection and onset days, and on the device the log's one launch a day records both.

`begin_numpy`, `record_numpy` and `report_numpy` are the executable specification: the library's kernels (k_course_begin,
k_course_day, k_course_report) compute the same words.  They go over ALL agents; k_course_day over the ACTIVE ones only, which
is the same thing (tests/test_course.py).  `run_host_driven` is the plain formulation, and what a Context on an engine library
without the entry points takes.

In line lists, -1 stands for NONE and -2 for BEFORE.
"""
import ctypes

import numpy as np

from . import engine as _eng
from . import reports as _rep
from . import txlog as _txl
from .txlog import BEFORE, NONE, check_n_days

COURSE_VERSION = 1             # include/reina_course.h: REINA_COURSE_VERSION
MAX_GROUPS, KINDS, DELAY_BINS, DETECTION_SHIFT, CLASSES, DAY_TABLES, COHORT_FIELDS = 16, 8, 64, 16, 10, 5, 4
F_DETECTION, F_ADMISSION, F_ICU, F_OUTCOME = 0, 16, 32, 48
DELAY = 0
DELAY_N = DELAY + KINDS * MAX_GROUPS * DELAY_BINS
DELAY_SUM = DELAY_N + KINDS * MAX_GROUPS
PATHWAY = DELAY_SUM + KINDS * MAX_GROUPS
SCALARS = PATHWAY + MAX_GROUPS * CLASSES
SCALAR_NAMES = ('infected', 'with_detection', 'with_admission', 'with_icu', 'with_outcome', 'detected_undated', 'out_of_range',
                'died_outside')
S_NR = 16
FIXED_WORDS = SCALARS + S_NR
DAY_WORDS = MAX_GROUPS * (DAY_TABLES + COHORT_FIELDS)
DAY_TABLE_NAMES = ('detections', 'admissions', 'icu_admissions', 'deaths', 'recoveries')
KIND_NAMES = ('onset_to_detection', 'onset_to_admission', 'admission_to_icu', 'ward_stay_recovered', 'ward_stay_dead',
              'icu_stay_recovered', 'icu_stay_dead', 'onset_to_death')
CLASS_NAMES = ('open_not_admitted', 'open_ward', 'open_icu', 'recovered_not_admitted', 'recovered_ward', 'recovered_icu',
               'died_not_admitted', 'died_ward', 'died_icu', 'undetermined')
S_HOSPITALIZED, S_IN_ICU, S_RECOVERED, S_DEAD = 3, 4, 5, 6   # csrc/reina_prims.h: RS_*
H_DETECTED, H_POD_OUTSIDE, H_ACTIVE = 0x40, 0x800, 0x8000    # csrc/reina_prims.h: RH_*

COURSE_FUNCTIONS = ('course_version', 'course_create', 'course_destroy', 'course_report', 'course_read', 'course_write')


def day_table_offset(k, n_days):
    """the word offset of the k-th table by day (DAY_TABLE_NAMES); k = DAY_TABLES: the cohorts"""
    return FIXED_WORDS + int(k) * int(n_days) * MAX_GROUPS


def report_words(n_days):
    """include/reina_course.h: REINA_COURSE_REPORT_WORDS"""
    return FIXED_WORDS + int(n_days) * DAY_WORDS


def bind_course_abi(lib, prefix):
    """The course log's entry points of a library, or None when it has none."""
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    args = {'course_create': [vp, vp, vp], 'course_destroy': [vp], 'course_report': [vp, vp, u32, u32, vp, vp],
            'course_read': [vp, u32, vp, vp], 'course_write': [vp, u32, vp, vp]}
    return _eng.bind_optional_abi(lib, prefix, COURSE_FUNCTIONS, args, 'course_version', COURSE_VERSION)


def pack(det, adm, icu, out):
    """records of four arrays of fields"""
    u = lambda x: np.asarray(x).astype(np.uint64) & np.uint64(0xFFFF)
    return u(det) | u(adm) << np.uint64(F_ADMISSION) | u(icu) << np.uint64(F_ICU) | u(out) << np.uint64(F_OUTCOME)


def fields(rec):
    """(detection, admission, icu, outcome) of an array of records, int64 each (codes as they are)"""
    r = np.asarray(rec, dtype=np.uint64).ravel()
    return tuple(((r >> np.uint64(b)) & np.uint64(0xFFFF)).astype(np.int64) for b in (F_DETECTION, F_ADMISSION, F_ICU, F_OUTCOME))


# ------------------------------------------------------------------------------------------------ the specification

def _conditions(hot):
    """(st, detected, admitted, in_icu, removed): what the hot words say of the four fields"""
    hot = np.asarray(hot).view(np.uint32).ravel()
    st = hot & 7
    return st, (hot & H_DETECTED) != 0, (st == S_HOSPITALIZED) | (st == S_IN_ICU), st == S_IN_ICU, st >= S_RECOVERED


def begin_numpy(hot):
    """the records of a state as the begin pass leaves them"""
    st, detected, admitted, in_icu, removed = _conditions(hot)
    code = lambda cond: np.where(removed | cond, BEFORE, NONE)
    return pack(code((st != 0) & detected), code(admitted), code(in_icu), code(False))


def record_numpy(rec, hot, day, where=None):
    """`rec` after day `day` has been recorded from the hot words as they stand after that day (a new array).  `where` (a
    mask): only these agents are looked at (k_course_day looks at the ACTIVE ones)."""
    day = int(day)
    if not 0 <= day < _eng.MAX_DAYS:
        raise ValueError('day %d: the course log holds days below %d' % (day, _eng.MAX_DAYS))
    st, detected, admitted, in_icu, removed = _conditions(hot)
    det, adm, icu, out = fields(rec)
    live = (out == NONE) & (st != 0)
    if where is not None:
        live &= np.asarray(where, dtype=bool)
    put = lambda f, cond: np.where(live & (f == NONE) & cond, day, f)
    return pack(put(det, detected), put(adm, admitted), put(icu, in_icu), put(out, removed))


def report_numpy(hot, log, rec, age_start, age_group, n_days):
    """The report of one state, its log and its records (the specification of reina_course_report).  hot: uint32[N]; log:
    uint32[N] (txlog.py); rec: uint64[N]; age_start: first agent of each age ([A] = N, padded with N); age_group: group of each
    age (< MAX_GROUPS); n_days: the tables by day hold the days [0, n_days)."""
    hot = np.asarray(hot).view(np.uint32).ravel()
    n_days = check_n_days(n_days)
    log = np.asarray(log, dtype=np.uint32).ravel()
    table, n_groups, _, age_of = _rep.age_lookup(age_start, age_group)
    words = np.zeros(report_words(n_days), dtype=np.uint64)
    idx = np.flatnonzero((hot & 7) != 0)
    w = hot[idx]
    st = w & 7
    g = table[age_of(idx)].astype(np.int64)
    t, o = (log[idx] & 0xFFFF).astype(np.int64), (log[idx] >> 16).astype(np.int64)
    det, adm, icu, out = fields(np.asarray(rec, dtype=np.uint64).ravel()[idx])
    known = lambda x: x < BEFORE
    dead, rcv = st == S_DEAD, st == S_RECOVERED
    ward, unit = known(out) & known(adm) & (icu == NONE), known(out) & known(icu)
    kinds = ((known(det) & known(o), det - o + DETECTION_SHIFT), (known(adm) & known(o), adm - o), (known(icu) & known(adm), icu - adm),
             (ward & rcv, out - adm), (ward & dead, out - adm), (unit & rcv, out - icu), (unit & dead, out - icu),
             (known(out) & known(o) & dead, out - o))
    sums = np.zeros(KINDS * MAX_GROUPS, dtype=np.int64)
    for k, (sel, val) in enumerate(kinds):
        cell = k * MAX_GROUPS + g[sel]
        words[DELAY:DELAY_N] += np.bincount(cell * DELAY_BINS + np.clip(val[sel], 0, DELAY_BINS - 1), minlength=DELAY_N - DELAY).astype(np.uint64)
        words[DELAY_N:DELAY_SUM] += np.bincount(cell, minlength=DELAY_SUM - DELAY_N).astype(np.uint64)
        np.add.at(sums, cell, val[sel])
    words[DELAY_SUM:PATHWAY] = sums.view(np.uint64)
    before = (adm == BEFORE) | (icu == BEFORE) | (out == BEFORE)
    determined = ~before & ((out == NONE) | dead | rcv)
    cls = np.where(determined, np.where(out == NONE, 0, np.where(rcv, 3, 6)) + np.where(known(icu), 2, np.where(known(adm), 1, 0)), 9)
    words[PATHWAY:SCALARS] = np.bincount(g * CLASSES + cls, minlength=SCALARS - PATHWAY).astype(np.uint64)

    def by_day(k, sel, day):
        sel = sel & known(day) & (day < n_days)
        a = day_table_offset(k, n_days)
        words[a:a + n_days * MAX_GROUPS] = np.bincount(day[sel] * MAX_GROUPS + g[sel], minlength=n_days * MAX_GROUPS).astype(np.uint64)

    everyone = np.ones(len(idx), dtype=bool)
    by_day(0, everyone, det)
    by_day(1, everyone, adm)
    by_day(2, everyone, icu)
    by_day(3, dead, out)
    by_day(4, rcv, out)
    inr = known(t) & (t < n_days)
    key = t[inr] * MAX_GROUPS + g[inr]
    coh = np.zeros((n_days * MAX_GROUPS, COHORT_FIELDS), dtype=np.uint64)
    for c, sel in enumerate((everyone, st >= S_RECOVERED, known(adm), dead)):
        coh[:, c] = np.bincount(key[sel[inr]], minlength=len(coh)).astype(np.uint64)
    words[day_table_offset(DAY_TABLES, n_days):] = coh.ravel()
    sc = dict(infected=len(idx), with_detection=int(known(det).sum()), with_admission=int(known(adm).sum()),
              with_icu=int(known(icu).sum()), with_outcome=int(known(out).sum()),
              detected_undated=int((((w & H_DETECTED) != 0) & (det == NONE)).sum()),
              out_of_range=sum(int((known(f) & (f >= n_days)).sum()) for f in (det, adm, icu, out)),
              died_outside=int((dead & ((w & H_POD_OUTSIDE) != 0)).sum()))
    for k, name in enumerate(SCALAR_NAMES):
        words[SCALARS + k] = sc[name]
    return CourseReport(words, n_days, n_groups)


# ------------------------------------------------------------------------------------------------ reports

class _Delay(_txl._Intervals):
    """an interval distribution whose mean is exact where the histogram clips: the count and the sum come with it"""

    def __init__(self, counts, shift, name, n, total):
        super().__init__(counts, shift, name)
        self.n, self.sum, self.shift = int(n), int(total), int(shift)

    def mean(self):
        """None when empty; exact: the sum was taken before clipping"""
        return self.sum / self.n - self.shift if self.n else None


class CourseReport(_rep.Report):
    """One report: the words of include/reina_course.h as named arrays, plus what is derived from them."""
    SCALARS, SCALAR_NAMES, IDENTITY = SCALARS, SCALAR_NAMES, ('n_days',)

    def __init__(self, words, n_days, n_groups=MAX_GROUPS, group_labels=None, start_date=None):
        self.n_days = n_days = int(n_days)
        w = self._take(words, report_words(n_days), 'a course report of %d days has %d words' % (n_days, report_words(n_days)),
                       n_groups, group_labels)
        self.start_date = start_date
        self.delay_counts = w[DELAY:DELAY_N].reshape(KINDS, MAX_GROUPS, DELAY_BINS)
        self.delay_n = w[DELAY_N:DELAY_SUM].reshape(KINDS, MAX_GROUPS)
        self.delay_sum = w[DELAY_SUM:PATHWAY].view(np.int64).reshape(KINDS, MAX_GROUPS)
        self.pathway = w[PATHWAY:SCALARS].reshape(MAX_GROUPS, CLASSES)
        for k, name in enumerate(DAY_TABLE_NAMES):
            a = day_table_offset(k, n_days)
            setattr(self, name, w[a:a + n_days * MAX_GROUPS].reshape(n_days, MAX_GROUPS))
        self.cohort = w[day_table_offset(DAY_TABLES, n_days):].reshape(n_days, MAX_GROUPS, COHORT_FIELDS)

    def __repr__(self):
        return 'CourseReport(days=%d, infected=%d, detected=%d, admitted=%d, icu=%d, closed=%d)' % (
            self.n_days, self.infected, self.with_detection, self.with_admission, self.with_icu, self.with_outcome)

    def _frame(self, table):
        import pandas as pd
        return pd.DataFrame(table[:, :self.n_groups].astype(np.int64), index=self._dates(), columns=pd.Index(self._groups(), name='age_group'))

    def detections_frame(self):
        """detections by date (rows) and age group (columns)"""
        return self._frame(self.detections)

    def admissions_frame(self):
        """hospital admissions by date and age group (an agent admitted straight to the ICU is admitted that day)"""
        return self._frame(self.admissions)

    def icu_admissions_frame(self):
        return self._frame(self.icu_admissions)

    def deaths_frame(self):
        return self._frame(self.deaths)

    def recoveries_frame(self):
        return self._frame(self.recoveries)

    def delay(self, kind, group=None):
        """One of KIND_NAMES ('onset_to_detection', 'onset_to_admission', 'admission_to_icu', 'onset_to_death', the four stays) as
        txlog's interval object -- counts by value, series(), quantile(), mean() -- of one age group or of all.  The mean is
        delay_sum / delay_n: exact although the end bins hold the clipped values."""
        k = KIND_NAMES.index(kind) if isinstance(kind, str) else int(kind)
        pick = (lambda a: a[k].sum(axis=0)) if group is None else (lambda a: a[k, int(group)])
        return _Delay(pick(self.delay_counts), DETECTION_SHIFT if k == 0 else 0, KIND_NAMES[k], pick(self.delay_n), pick(self.delay_sum))

    def length_of_stay(self, where, outcome, group=None):
        """days from admission to the outcome of those who never reached the ICU ('ward'), or from ICU admission to the outcome
        ('icu'); outcome 'recovered' or 'dead'"""
        if where not in ('ward', 'icu') or outcome not in ('recovered', 'dead'):
            raise ValueError("length_of_stay('ward' | 'icu', 'recovered' | 'dead')")
        return self.delay('%s_stay_%s' % (where, outcome), group)

    def pathways_frame(self):
        """infected agents by age group (rows) and pathway through care (CLASS_NAMES)"""
        import pandas as pd
        return pd.DataFrame(self.pathway[:self.n_groups].astype(np.int64), index=pd.Index(self._groups(), name='age_group'),
                            columns=list(CLASS_NAMES))

    def _by_cohort(self, field, name, group):
        import pandas as pd
        c = (self.cohort.sum(axis=1, dtype=np.uint64) if group is None else self.cohort[:, int(group)]).astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio, closed = c[:, field] / c[:, 0], c[:, 1] / c[:, 0]
        return pd.DataFrame({name: ratio, 'cohort': c[:, 0].astype(np.int64), 'closed_share': closed}, index=self._dates())

    def fatality_by_cohort(self, group=None):
        """by date of infection: the share of the cohort that has died so far (NaN for an empty cohort), the cohort's size and the
        share of it that is removed (the ratio of an open cohort is censored)"""
        return self._by_cohort(3, 'ifr', group)

    def hospitalisation_by_cohort(self, group=None):
        """by date of infection: the share of the cohort with a known admission day, the cohort's size, its closed share"""
        return self._by_cohort(2, 'hospitalised', group)


# ------------------------------------------------------------------------------------------------ course logs

class DeviceCourse(_eng.Handle):
    """The library's course log of a txlog.DeviceLog: of one engine, or of the members of an engine group."""
    DESTROY = 'course_destroy'
    group = property(lambda self: self.log.group)       # (with `engines`: what reports.device_take reads of a log on the device)
    engines = property(lambda self: self.log.engines)

    def __init__(self, device_log):
        e = device_log.engine
        self.f = f = _rep.entry_points(e, 'course_f', 'course-log', 'reina_course.h')
        if device_log.course is not None:
            raise ValueError('this transmission log has a course log attached already')
        self.log, self.engine, self.members = device_log, e, device_log.members
        self._h = ctypes.c_void_p()
        e._check(f['course_create'](device_log._h, e.alloc.stream(), ctypes.byref(self._h)), 'course_create')
        device_log.course = self

    def _closing(self):
        if self.log.course is self:
            self.log.course = None

    def words(self, member=0):
        out = np.zeros(self.engine.config.n_agents, dtype=np.uint64)
        self.engine._check(self.f['course_read'](self._h, int(member), out.ctypes.data, self.engine.alloc.stream()), 'course_read')
        return out

    def set_words(self, words, member=0):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if len(w) != self.engine.config.n_agents:
            raise ValueError('a course log has one record per agent')
        self.engine._check(self.f['course_write'](self._h, int(member), w.ctypes.data, self.engine.alloc.stream()), 'course_write')


class CourseLog:
    """The course log of one Context (ctx.course_log), attached to its transmission log and kept where that is kept: on the
    device (the log's launch of the day records both) or in host memory.  A member of a logged engine group shares the
    group's DeviceCourse (`device`, `member`)."""

    def __init__(self, ctx, device=None, member=0):
        log = ctx.transmission_log
        if log is None:
            raise ValueError('a course log is attached to a transmission log: this Context keeps none')
        if log.course is not None:
            raise ValueError('start_course_log: this Context keeps a course log already')
        self.ctx, self.log, self.member = ctx, log, int(member)
        self.begin_day = int(ctx.day)
        self.device, self._words = device, None
        if device is None:
            if log.on_device:
                self.device = DeviceCourse(log.device)
            else:
                self._words = begin_numpy(_txl._host_array(ctx.engine.tensors['hot']))
        log.course = self

    @property
    def on_device(self):
        return self.device is not None

    def close(self):
        if self.device is not None and self.device.log.group is None:
            self.device.close()
        if self.log.course is self:
            self.log.course = None

    def record_host(self, hot, day):
        """the host-side records after day `day` (the log calls it behind its own update; a device course is recorded by the
        log's launch)"""
        if self.device is None:
            self._words = record_numpy(self._words, hot, day)

    def words(self):
        """uint64[n_agents], a host copy"""
        return self.device.words(self.member) if self.device is not None else self._words.copy()

    def set_words(self, words):
        if self.device is not None:
            self.device.set_words(words, self.member)
        else:
            self._words = np.array(words, dtype=np.uint64)

    def days(self):
        """(detection, admission, icu, outcome) days, int64[n_agents] each: -1 NONE, -2 BEFORE"""
        return tuple(_txl._signed(f) for f in fields(self.words()))

    def report(self, age_groups=None, n_days=None):
        """CourseReport of the days [0, n_days) (default: the days run so far)"""
        return _rep.report_of(COURSE, self, age_groups, n_days)

    def detection_report(self, age_groups=None, n_days=None):
        """detection.DetectionReport of the days [0, n_days) (default: the days run so far): ascertainment by age, severity and
        date of infection, transmission from agents never detected and before a detection, lead times, and what tracing adds.
        One launch where the course is a single engine's on the device and the library has the entry points,
        detection.report_numpy on host copies otherwise.  Reads the engine's state, the log and the course only."""
        from . import detection as _det
        return _det.report_course(self, age_groups, n_days)


def run_host_driven(ctx, days, record_history=True, on_day=None):
    """txlog.run_host_driven with the course kept beside the log: per day iterate(), read the hot words back, record both --
    on any engine.  Begins a host-side log and course when the Context has none.  on_day(day, hot, records_before,
    records_after), when given, is called after every day (the tests' handle)."""
    if ctx.transmission_log is None:
        ctx.transmission_log = _txl.TransmissionLog(ctx, host=True)
    if ctx.course_log is None:
        ctx.course_log = CourseLog(ctx)
    course = ctx.course_log
    if course.on_device:
        raise ValueError('run_host_driven: this Context keeps its course log on the device')
    state = [course._words]

    def each(day, hot, log_before, log_after):   # (txlog.run_host_driven has recorded the course by now)
        before, state[0] = state[0], course._words
        if on_day is not None:
            on_day(day, hot, before, course._words)

    return _txl.run_host_driven(ctx, days, record_history, each)


COURSE = _rep.Kind(
    name='course_reports', of='course_log', arguments=_txl.day_arguments, report=CourseReport, words=report_words,
    numpy=lambda ctx, course, table, params: lambda depth: report_numpy(_rep.host_state(ctx.engine)[0], course.log.words(), course.words(),
                                                                         ctx.age_start, table, *params).words,
    names=('course_report', 'course_report'), on=lambda glog: glog.course)


def report_group(device_course, contexts, age_groups=None, n_days=None):
    """The reports of every member of a group's course log (or of the one engine of a device course): one launch for all."""
    return _rep.reports_of_device(COURSE, device_course, contexts, age_groups, n_days)
