"""A detection report: what share of the infections is ever found, how much transmission comes from agents that are never found
or not found yet, and what contact tracing adds (include/reina_detection.h).

Testing and tracing act on the epidemic through one mechanism: a detected agent is quarantined and exposes nobody.  The
course log (course.py) dates every detection, the transmission log (txlog.py) every infection, and the cold record names every
agent's infector.  A report joins the three, between two days, and changes nothing.  With w an agent's hot word, st = w & 7,
sev = (w >> 3) & 7, DETECTED = w & 0x40, t and o the log's days, det / adm / out the record's fields (KNOWN when neither code):

  detection class dc   1 dated    det known
                       2 before   det BEFORE (detected before the course began, or removed by then whether detected or not)
                       3 undated  det NONE and DETECTED (the detection reached the agent after its record closed)
                       0 never    det NONE and not DETECTED
  phase at detection   of dc == 1, the first that applies: 0 before onset (o NONE, or o known and det < o), 1 at admission (adm
                       known, det == adm), 2 ill, in the community (o known, and adm NONE or det < adm known), 3 undetermined
  link class           of a link s -> i (reports.links), the first that applies: 0 infector never detected (dc(s) == 0),
                       4 undetermined (dc(s) 2 or 3, or t(i) not known), 1 before detection (t(i) < det(s)), 2 same day,
                       3 after -- a breach of the quarantine, which no simulated state holds

`report_numpy` is the executable specification, over all agents and links: the library's kernel (k_detect_report) computes the
same words.  A report is a function of the state, the log and the course alone, so the host route -- report_numpy on host
copies, what oracle B, a host-kept log and a group's member taken alone take -- and the device route agree word for word.
"""
import collections
import ctypes

import numpy as np

from . import course as _crs
from . import engine as _eng
from . import reports as _rep
from . import txlog as _txl
from .txlog import BEFORE, NONE, check_n_days

DETECT_VERSION = 1             # include/reina_detection.h: REINA_DETECT_VERSION
MAX_GROUPS, SEVERITIES, CLASSES, PHASES, LINK_CLASSES, BINS, PAIR_BINS, PAIR_SHIFT = 16, 8, 4, 4, 5, 64, 128, 64
COHORT_FIELDS, LINK_DAY_FIELDS = 3, 3
NEVER, DATED, BEFORE_COURSE, UNDATED = 0, 1, 2, 3
ASCERTAIN = 0
PHASE = ASCERTAIN + MAX_GROUPS * SEVERITIES * CLASSES
AT_LARGE = PHASE + MAX_GROUPS * PHASES
AT_LARGE_N = AT_LARGE + MAX_GROUPS * BINS
AT_LARGE_SUM = AT_LARGE_N + MAX_GROUPS
OFFSPRING = AT_LARGE_SUM + MAX_GROUPS
OFFSPRING_SUM = OFFSPRING + CLASSES * 2 * BINS
LINK_CLASS = OFFSPRING_SUM + CLASSES * 2
LEAD = LINK_CLASS + MAX_GROUPS * LINK_CLASSES
PAIR = LEAD + MAX_GROUPS * BINS
PAIR_CLASS = PAIR + PAIR_BINS
SCALARS = PAIR_CLASS + CLASSES * CLASSES
SCALAR_NAMES = ('infected', 'roots', 'linked', 'bad_links', 'never', 'dated', 'before', 'undated', 'breach', 'out_of_range')
S_NR = 16
FIXED_WORDS = SCALARS + S_NR
DAY_WORDS = MAX_GROUPS * COHORT_FIELDS + PHASES + LINK_DAY_FIELDS
CLASS_NAMES = ('never', 'dated', 'before', 'undated')
PHASE_NAMES = ('before_onset', 'at_admission', 'ill_in_community', 'undetermined')
LINK_CLASS_NAMES = ('infector_never_detected', 'before_detection', 'same_day', 'after_detection', 'undetermined')
SEVERITY_NAMES = ('asymptomatic', 'mild', 'severe', 'critical', 'fatal', '5', '6', '7')
S_RECOVERED = 5                # csrc/reina_prims.h: RS_RECOVERED
H_DETECTED = 0x40              # csrc/reina_prims.h: RH_DETECTED

DETECT_FUNCTIONS = ('detect_version', 'detect_report')


def cohort_offset(n_days):
    return FIXED_WORDS


def detections_offset(n_days):
    return cohort_offset(n_days) + int(n_days) * MAX_GROUPS * COHORT_FIELDS


def links_by_day_offset(n_days):
    return detections_offset(n_days) + int(n_days) * PHASES


def report_words(n_days):
    """include/reina_detection.h: REINA_DETECT_REPORT_WORDS"""
    return FIXED_WORDS + int(n_days) * DAY_WORDS


def bind_detect_abi(lib, prefix):
    """The detection report's entry points of a library, or None when it has none."""
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    return _eng.bind_optional_abi(lib, prefix, DETECT_FUNCTIONS, {'detect_report': [vp, vp, u32, u32, vp, vp]}, 'detect_version', DETECT_VERSION)


# ------------------------------------------------------------------------------------------------ the specification

def _classes(det, hot):
    """the detection class of arrays of detection fields and hot words"""
    return np.where(det < BEFORE, DATED, np.where(det == BEFORE, BEFORE_COURSE, np.where((hot & H_DETECTED) != 0, UNDATED, NEVER))).astype(np.int64)


def report_numpy(hot, infector, n_infected, log, rec, age_start, age_group, n_days):
    """The report of one state, its log and its course records (the specification of reina_detect_report).  hot: uint32[N];
    infector: int32[N] and n_infected: uint32[N] (the cold record's fields; looked at only of infected agents); log: uint32[N]
    (txlog.py); rec: uint64[N] (course.py); age_start: first agent of each age ([A] = N, padded with N); age_group: group of
    each age (< MAX_GROUPS); n_days: the tables by day hold the days [0, n_days)."""
    hot = np.asarray(hot).view(np.uint32).ravel()
    n_days = check_n_days(n_days)
    log = np.asarray(log, dtype=np.uint32).ravel()
    rec = np.asarray(rec, dtype=np.uint64).ravel()
    table, n_groups, _, age_of = _rep.age_lookup(age_start, age_group)
    words = np.zeros(report_words(n_days), dtype=np.uint64)
    count = lambda cells, size: np.bincount(cells, minlength=size).astype(np.uint64)
    k = _rep.links(hot, infector)
    idx = k.idx
    w = hot[idx]
    st, sev = (w & 7).astype(np.int64), ((w >> 3) & 7).astype(np.int64)
    n = np.asarray(n_infected).view(np.uint32).ravel()[idx].astype(np.int64)
    g = table[age_of(idx)].astype(np.int64)
    t, o = (log[idx] & 0xFFFF).astype(np.int64), (log[idx] >> 16).astype(np.int64)
    det, adm, _, _ = _crs.fields(rec[idx])
    known = lambda x: x < BEFORE
    tk, closed = known(t), st >= S_RECOVERED
    dc = _classes(det, w)
    dated = dc == DATED
    ph = np.where((o == NONE) | (known(o) & (det < o)), 0,
                  np.where(known(adm) & (det == adm), 1,
                           np.where(known(o) & ((adm == NONE) | (known(adm) & (det < adm))), 2, 3)))
    words[ASCERTAIN:PHASE] = count((g * SEVERITIES + sev) * CLASSES + dc, PHASE - ASCERTAIN)
    words[PHASE:AT_LARGE] = count((g * PHASES + ph)[dated], AT_LARGE - PHASE)
    large = dated & tk
    days = det - t
    words[AT_LARGE:AT_LARGE_N] = count((g * BINS + np.clip(days, 0, BINS - 1))[large], AT_LARGE_N - AT_LARGE)
    words[AT_LARGE_N:AT_LARGE_SUM] = count(g[large], MAX_GROUPS)
    sums = np.zeros(MAX_GROUPS, dtype=np.int64)
    np.add.at(sums, g[large], days[large])
    words[AT_LARGE_SUM:OFFSPRING] = sums.view(np.uint64)
    oc = dc * 2 + closed
    words[OFFSPRING:OFFSPRING_SUM] = count(oc * BINS + np.minimum(n, BINS - 1), OFFSPRING_SUM - OFFSPRING)
    osum = np.zeros(CLASSES * 2, dtype=np.int64)
    np.add.at(osum, oc, n)
    words[OFFSPRING_SUM:LINK_CLASS] = osum.view(np.uint64)
    # the links: i over the linked agents, s their infectors
    li = np.flatnonzero(k.linked)
    s = k.s[li]
    ws = hot[s]
    dets = _crs.fields(rec[s])[0]
    dcs = _classes(dets, ws)
    gs = table[age_of(s)].astype(np.int64)
    ti, tik, dci, deti = t[li], tk[li], dc[li], det[li]
    cls = np.where(dcs == NEVER, 0, np.where((dcs != DATED) | ~tik, 4, np.where(ti < dets, 1, np.where(ti == dets, 2, 3))))
    ahead = (cls == 1) | (cls == 2)
    words[LINK_CLASS:LEAD] = count(gs * LINK_CLASSES + cls, LEAD - LINK_CLASS)
    words[LEAD:PAIR] = count((gs * BINS + np.clip(dets - ti, 0, BINS - 1))[ahead], PAIR - LEAD)
    both = (dcs == DATED) & (dci == DATED)
    words[PAIR:PAIR_CLASS] = count(np.clip(deti - dets + PAIR_SHIFT, 0, PAIR_BINS - 1)[both], PAIR_BINS)
    words[PAIR_CLASS:SCALARS] = count(dcs * CLASSES + dci, CLASSES * CLASSES)
    # the tables by day
    a, b, c = cohort_offset(n_days), detections_offset(n_days), links_by_day_offset(n_days)
    tin = tk & (t < n_days)
    coh = np.zeros((n_days * MAX_GROUPS, COHORT_FIELDS), dtype=np.uint64)
    key = t * MAX_GROUPS + g
    for f, sel in enumerate((tin, tin & (dc != NEVER), tin & closed)):
        coh[:, f] = count(key[sel], len(coh))
    words[a:b] = coh.ravel()
    din = dated & (det < n_days)
    words[b:c] = count((det * PHASES + ph)[din], c - b)
    lin = tin[li]
    lbd = np.zeros((n_days, LINK_DAY_FIELDS), dtype=np.uint64)
    for f, sel in enumerate((lin, lin & (cls == 0), lin & ahead)):
        lbd[:, f] = count(ti[sel], n_days)
    words[c:] = lbd.ravel()
    by_class = np.bincount(dc, minlength=CLASSES)
    sc = dict(infected=len(idx), roots=int(k.root.sum()), linked=int(k.linked.sum()), bad_links=int(k.bad.sum()),
              never=int(by_class[NEVER]), dated=int(by_class[DATED]), before=int(by_class[BEFORE_COURSE]), undated=int(by_class[UNDATED]),
              breach=int((cls == 3).sum()), out_of_range=int((tk & (t >= n_days)).sum()) + int((dated & (det >= n_days)).sum()))
    for j, name in enumerate(SCALAR_NAMES):
        words[SCALARS + j] = sc[name]
    return DetectionReport(words, n_days, n_groups)


# ------------------------------------------------------------------------------------------------ reports

Share = collections.namedtuple('Share', 'share count total')


def _ratio(a, b):
    """a / b, None when b is 0 (an empty class has no share)"""
    return int(a) / int(b) if int(b) else None


def _class(dc):
    return CLASS_NAMES.index(dc) if isinstance(dc, str) else int(dc)


class DetectionReport(_rep.Report):
    """One report: the words of include/reina_detection.h as named arrays, plus what is derived from them."""
    SCALARS, SCALAR_NAMES, IDENTITY = SCALARS, SCALAR_NAMES, ('n_days',)

    def __init__(self, words, n_days, n_groups=MAX_GROUPS, group_labels=None, start_date=None):
        self.n_days = n_days = int(n_days)
        w = self._take(words, report_words(n_days), 'a detection report of %d days has %d words' % (n_days, report_words(n_days)),
                       n_groups, group_labels)
        self.start_date = start_date
        self.ascertain = w[ASCERTAIN:PHASE].reshape(MAX_GROUPS, SEVERITIES, CLASSES)
        self.phase = w[PHASE:AT_LARGE].reshape(MAX_GROUPS, PHASES)
        self.at_large = w[AT_LARGE:AT_LARGE_N].reshape(MAX_GROUPS, BINS)
        self.at_large_n = w[AT_LARGE_N:AT_LARGE_SUM]
        self.at_large_sum = w[AT_LARGE_SUM:OFFSPRING].view(np.int64)
        self.offspring = w[OFFSPRING:OFFSPRING_SUM].reshape(CLASSES, 2, BINS)
        self.offspring_sum = w[OFFSPRING_SUM:LINK_CLASS].reshape(CLASSES, 2)
        self.link_class = w[LINK_CLASS:LEAD].reshape(MAX_GROUPS, LINK_CLASSES)
        self.lead = w[LEAD:PAIR].reshape(MAX_GROUPS, BINS)
        self.pair = w[PAIR:PAIR_CLASS]
        self.pair_class = w[PAIR_CLASS:SCALARS].reshape(CLASSES, CLASSES)
        a, b, c = cohort_offset(n_days), detections_offset(n_days), links_by_day_offset(n_days)
        self.cohort = w[a:b].reshape(n_days, MAX_GROUPS, COHORT_FIELDS)
        self.detections = w[b:c].reshape(n_days, PHASES)
        self.links_by_day = w[c:].reshape(n_days, LINK_DAY_FIELDS)

    def __repr__(self):
        return 'DetectionReport(days=%d, infected=%d, never=%d, dated=%d, before=%d, undated=%d, links=%d, breach=%d)' % (
            self.n_days, self.infected, self.never, self.dated, self.before, self.undated, self.linked, self.breach)

    # ---- ascertainment

    def ascertainment_frame(self):
        """by age group and severity (rows): the share of the infected agents that were ever detected (dc != 0; None -> NaN for
        an empty cell), with the detected and the infected counts"""
        import pandas as pd
        a = self.ascertain[:self.n_groups].astype(np.int64)
        total, found = a.sum(axis=2), a[:, :, 1:].sum(axis=2)
        with np.errstate(divide='ignore', invalid='ignore'):
            share = found / total.astype(np.float64)
        index = pd.MultiIndex.from_product([self._groups(), SEVERITY_NAMES], names=['age_group', 'severity'])
        return pd.DataFrame({'share': share.ravel(), 'detected': found.ravel(), 'infected': total.ravel()}, index=index)

    def ascertainment_by_cohort(self, group=None):
        """by date of infection: the share of the cohort detected so far (NaN for an empty cohort), the cohort's size and the
        share of it that is removed -- an open cohort's ratio is censored, as course.fatality_by_cohort's"""
        import pandas as pd
        c = (self.cohort.sum(axis=1, dtype=np.uint64) if group is None else self.cohort[:, int(group)]).astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio, closed = c[:, 1] / c[:, 0], c[:, 2] / c[:, 0]
        return pd.DataFrame({'ascertained': ratio, 'cohort': c[:, 0].astype(np.int64), 'closed_share': closed}, index=self._dates())

    def detections_frame(self):
        """dated detections by date (rows) and phase at detection (columns)"""
        import pandas as pd
        return pd.DataFrame(self.detections.astype(np.int64), index=self._dates(), columns=pd.Index(PHASE_NAMES, name='phase'))

    def phase_frame(self):
        """dated detections by age group (rows) and phase at detection"""
        import pandas as pd
        return pd.DataFrame(self.phase[:self.n_groups].astype(np.int64), index=pd.Index(self._groups(), name='age_group'),
                            columns=pd.Index(PHASE_NAMES, name='phase'))

    def days_at_large(self, group=None):
        """days from the infection to the detection of the agents with both days known, as course's interval object -- counts by
        value, series(), quantile() and the exact mean (the sum was taken before clipping) -- of one age group or of all"""
        pick = (lambda x: x.sum(axis=0)) if group is None else (lambda x: x[int(group)])
        return _crs._Delay(pick(self.at_large), 0, 'days_at_large', pick(self.at_large_n), pick(self.at_large_sum))

    # ---- transmission by detection class

    def offspring_by_detection(self):
        """by detection class (rows): the mean number of agents infected, the agents and their offspring -- of all agents and of
        the closed ones (NaN for an empty class)"""
        import pandas as pd
        agents = self.offspring.sum(axis=2).astype(np.int64)        # [dc, closed]
        total = self.offspring_sum.astype(np.int64)
        cols = {}
        for name, ag, tot in (('all', agents.sum(axis=1), total.sum(axis=1)), ('closed', agents[:, 1], total[:, 1])):
            with np.errstate(divide='ignore', invalid='ignore'):
                cols[(name, 'mean')] = tot / ag.astype(np.float64)
            cols[(name, 'agents')], cols[(name, 'offspring')] = ag, tot
        return pd.DataFrame(cols, index=pd.Index(CLASS_NAMES, name='detection'))

    def transmission_share(self, dc='never', closed_only=False):
        """Share(share, count, total): the share of all infections made (the sum of n) that agents of one detection class made --
        'never': the transmission testing did not see -- with the two sums.  closed_only: over the removed agents only (an open
        case may yet be detected, so 'never' is censored in an open epidemic).  None when nobody infected anyone."""
        s = self.offspring_sum[:, 1] if closed_only else self.offspring_sum.sum(axis=1)
        part, total = int(s[_class(dc)]), int(s.sum())
        return Share(_ratio(part, total), part, total)

    def link_frame(self):
        """links by the infector's age group (rows) and link class"""
        import pandas as pd
        return pd.DataFrame(self.link_class[:self.n_groups].astype(np.int64), index=pd.Index(self._groups(), name='age_group'),
                            columns=pd.Index(LINK_CLASS_NAMES, name='link_class'))

    def lead_time(self, group=None):
        """days from a transmission to its infector's detection, of the links made before or on that day (classes 1 and 2), as
        txlog's interval object; the last bin holds the clipped values.  group: the infector's"""
        counts = self.lead.sum(axis=0, dtype=np.uint64) if group is None else self.lead[int(group)]
        return _txl._Intervals(counts, 0, 'lead_days')

    def averted_if_earlier(self, k):
        """Share(share, count, total): the share of the links of class 1 and 2 made 1 .. k days before their infector's
        detection -- what a detection k days earlier would have cut off.  FIRST ORDER only: it ignores the chains behind an
        averted link (their descendants would not have been infected either) and every knock-on effect.  None without such links."""
        k = int(k)
        if k < 0:
            raise ValueError('averted_if_earlier: k must not be negative')
        c = self.lead.sum(axis=0, dtype=np.uint64)
        part, total = int(c[1:min(k, BINS - 1) + 1].sum()), int(c.sum())
        return Share(_ratio(part, total), part, total)

    # ---- tracing

    def pair_detection(self):
        """det(infectee) - det(infector) of the links with both detections dated, as txlog's interval object (values -64 .. 63,
        the end bins clipped)"""
        return _txl._Intervals(self.pair, PAIR_SHIFT, 'pair_days')

    def adjacent_share(self, d=1):
        """the share of the dated pairs detected exactly d days apart, either way round (tracing finds an infectee the day
        after its infector); None without dated pairs"""
        d = abs(int(d))
        if not 0 <= d < PAIR_SHIFT:
            raise ValueError('adjacent_share: |d| must be below %d' % PAIR_SHIFT)
        p = self.pair.astype(np.int64)
        part = int(p[PAIR_SHIFT]) if d == 0 else int(p[PAIR_SHIFT + d]) + int(p[PAIR_SHIFT - d])
        return _ratio(part, p.sum())

    def pair_frame(self):
        """links by the infector's detection class (rows) and the infectee's (columns)"""
        import pandas as pd
        return pd.DataFrame(self.pair_class.astype(np.int64), index=pd.Index(CLASS_NAMES, name='infector'), columns=pd.Index(CLASS_NAMES, name='infectee'))

    def links_frame(self):
        """by date of transmission: links, those from never-detected infectors and from infectors not detected yet, and the
        share from never-detected ones (NaN on a day without links).  An open epidemic CENSORS 'never': an infector still ill
        may yet be detected, so the share of the last weeks overstates it."""
        import pandas as pd
        m = self.links_by_day.astype(np.int64)
        with np.errstate(divide='ignore', invalid='ignore'):
            share = m[:, 1] / m[:, 0].astype(np.float64)
        return pd.DataFrame({'links': m[:, 0], 'never_detected': m[:, 1], 'before_detection': m[:, 2], 'never_share': share}, index=self._dates())


# ------------------------------------------------------------------------------------------------ routes

def _numpy_route(ctx, course, table, params):
    def take(depth):
        hot, infector, n_infected, _ = _rep.host_state(ctx.engine)
        return report_numpy(hot, infector, n_infected, course.log.words(), course.words(), ctx.age_start, table, *params).words
    return take


DETECTION = _rep.Kind(
    name='detection_reports', of='course_log', arguments=_txl.day_arguments, report=DetectionReport, words=report_words,
    numpy=_numpy_route, names=('detect_report', 'detect_report'), on=lambda glog: glog.course,
    entry=('detect_f', 'detection report', 'reina_detection.h'))


def device_report_words(device_course, table, n_groups, n_days):
    """[members, report_words(n_days)] uint64 of a course.DeviceCourse: one launch for all members"""
    return _rep.device_take(DETECTION, device_course, table, n_groups, (n_days,))()


def report_course(course_log, age_groups=None, n_days=None):
    """CourseLog.detection_report (reports.report_of)"""
    return _rep.report_of(DETECTION, course_log, age_groups, n_days)
