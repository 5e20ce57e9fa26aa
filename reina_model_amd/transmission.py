"""Transmission-tree reports: who infected whom, as exact integer counts (include/reina_transmission.h; DESIGN.md
"Transmission reports").

The engine keeps every agent's true infector and its number of secondary infections.  A report, taken between two days of an
unsharded engine, counts them into: the offspring distribution by variant, severity, outcome and detection; exact sums of
n_infected and of its square; the infector-age x infectee-age matrix; the generation histogram; and the cluster sizes of the
trees that grow from each root (imports and the initial condition).

`report_numpy` is the executable specification: the library's kernels (reina_tx_report) compute the same words.  It is also
the path of engines whose state lives in host memory (engine.NumpyAllocator).
"""
import ctypes

import numpy as np

from . import engine as _eng
from . import reports as _rep
from .reports import _group_table, default_age_groups, rounds_for  # noqa: F401  (theirs since reports.py; used from here)

TX_VERSION = 1                 # include/reina_transmission.h: REINA_TX_VERSION
VARIANTS, SEVERITIES, OUTCOMES, BINS = 4, 5, 3, 64
MAX_GROUPS = 16
GENERATIONS = 256
CLUSTER_BINS = 33
OFFSPRING = 0
OFFSPRING_SUM = OFFSPRING + VARIANTS * SEVERITIES * OUTCOMES * 2 * BINS
OFFSPRING_SUMSQ = OFFSPRING_SUM + VARIANTS * OUTCOMES
MATRIX = OFFSPRING_SUMSQ + VARIANTS * OUTCOMES
GENERATION = MATRIX + VARIANTS * MAX_GROUPS * MAX_GROUPS
CLUSTERS = GENERATION + VARIANTS * GENERATIONS
CLUSTER_AGENTS = CLUSTERS + CLUSTER_BINS
SCALARS = CLUSTER_AGENTS + CLUSTER_BINS
SCALAR_NAMES = ('n_infected_agents', 'n_roots', 'n_linked', 'sum_n_infected', 'max_generation', 'largest_cluster',
                'largest_root', 'bad_links', 'unconverged', 'rounds', 'largest_key')
S_NR = 16
REPORT_WORDS = SCALARS + S_NR
OUTCOME_NAMES = ('active', 'counted', 'removed_uncounted')
SEVERITY_NAMES = ('asymptomatic', 'mild', 'severe', 'critical', 'fatal')

TX_FUNCTIONS = ('tx_version', 'tx_report', 'group_tx_report')


def scratch_bytes(n_agents):
    """include/reina_transmission.h: REINA_TX_SCRATCH_BYTES"""
    return (int(n_agents) * 20 + 255) & ~255


def bind_tx_abi(lib, prefix):
    """The transmission-report entry points of a library, or None when it has none."""
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    argtypes = {'tx_report': [vp, vp, u32, u32, vp, vp, vp], 'group_tx_report': [vp, vp, u32, u32, vp, vp, vp]}
    return _eng.bind_optional_abi(lib, prefix, TX_FUNCTIONS, argtypes, 'tx_version', TX_VERSION)


def report_numpy(hot, infector, n_infected, age_start, age_group, max_depth=None):
    """The report of one state (the specification of reina_tx_report).  hot: uint32[N]; infector, n_infected: int32[N] (the
    cold record's fields); age_start: first agent of each age ([A] = N, padded with N); age_group: group of each age
    (< MAX_GROUPS); max_depth: the deepest generation resolved (None: N, which every chain without a cycle fits)."""
    hot = np.asarray(hot).view(np.uint32).ravel()
    n = len(hot)
    cnt = np.asarray(n_infected).view(np.uint32).ravel().astype(np.uint64)
    table, n_groups, _, ages = _rep.age_lookup(age_start, age_group)
    rounds = rounds_for(n if max_depth is None else max_depth)

    words = np.zeros(REPORT_WORDS, dtype=np.uint64)
    _, idx, s, root, linked, bad = _rep.links(hot, infector)
    w = hot[idx]
    v = ((w >> 8) & 3).astype(np.int64)
    sev = np.minimum((w >> 3) & 7, 4).astype(np.int64)
    out = np.where((w & 7) <= 4, 0, np.where(w & 0x400, 1, 2)).astype(np.int64)
    det = ((w & 0x40) != 0).astype(np.int64)
    c = cnt[idx]
    cell = (((v * SEVERITIES + sev) * OUTCOMES + out) * 2 + det) * BINS + np.minimum(c, BINS - 1).astype(np.int64)
    words[OFFSPRING:OFFSPRING_SUM] = np.bincount(cell, minlength=OFFSPRING_SUM - OFFSPRING).astype(np.uint64)
    vo = v * OUTCOMES + out
    for k in range(VARIANTS * OUTCOMES):
        sel = c[vo == k]
        words[OFFSPRING_SUM + k] = int(sel.sum(dtype=np.uint64))
        words[OFFSPRING_SUMSQ + k] = int((sel * sel).sum(dtype=np.uint64))

    li = idx[linked]
    gs, gi = table[ages(li)].astype(np.int64), table[ages(s[linked])].astype(np.int64)
    words[MATRIX:GENERATION] = np.bincount((v[linked] * MAX_GROUPS + gi) * MAX_GROUPS + gs,
                                           minlength=GENERATION - MATRIX).astype(np.uint64)

    p, gen, conv = _rep.forest(n, idx, s, linked, rounds)
    words[GENERATION:CLUSTERS] = np.bincount(v[conv] * GENERATIONS + np.minimum(gen[conv], GENERATIONS - 1),
                                             minlength=CLUSTERS - GENERATION).astype(np.uint64)
    size = np.bincount(p[conv], minlength=n)
    roots = np.flatnonzero(size)
    rs = size[roots].astype(np.int64)
    b = np.floor(np.log2(np.maximum(rs, 1))).astype(np.int64)
    words[CLUSTERS:CLUSTER_AGENTS] = np.bincount(b, minlength=CLUSTER_BINS).astype(np.uint64)
    words[CLUSTER_AGENTS:SCALARS] = np.bincount(b, weights=rs, minlength=CLUSTER_BINS).astype(np.uint64)
    sc = dict(n_infected_agents=len(idx), n_roots=int(root.sum()), n_linked=int(linked.sum()),
              sum_n_infected=int(words[OFFSPRING_SUM:OFFSPRING_SUMSQ].sum(dtype=np.uint64)),
              max_generation=int(gen[conv].max()) if conv.any() else 0, bad_links=int(bad.sum()),
              unconverged=int((~conv).sum()), rounds=rounds)
    sc['largest_cluster'], sc['largest_root'], sc['largest_key'] = _rep.largest(roots, rs)
    for k, name in enumerate(SCALAR_NAMES):
        words[SCALARS + k] = sc[name]
    return TransmissionReport(words, n_groups)


def _check_unsharded(config):
    if config.n_shards > 1 or config.exact_attribution:
        raise ValueError('transmission reports are taken of unsharded engines only')


_UNCONVERGED = SCALARS + SCALAR_NAMES.index('unconverged')


def _device_reports(engines, group, age_group, n_groups):
    """the reports of `engines` by the library's kernels, one launch per pass: the members of `group`, or one engine (None)"""
    e0 = engines[0]
    for e in engines:
        _check_unsharded(e.config)
    table, ng = _group_table(age_group, e0.config.nr_ages)
    ng = max(ng, int(n_groups or 0))
    f = _rep.entry_points(e0, 'tx_f', 'transmission-report', 'reina_transmission.h')
    name, handle = ('tx_report', e0._h) if group is None else ('group_tx_report', group._h)
    n = e0.config.n_agents            # (of every member: an engine group is made of engines of one population)
    take = lambda depth: _rep.device_words(e0, f, name, (handle, table.ctypes.data, ng, int(depth or 0)), len(engines), REPORT_WORDS,
                                           scratch_bytes(n), engines, group is not None)
    return [TransmissionReport(w, ng) for w in _rep.member_rows(_rep.with_deep_pass(take, _UNCONVERGED, n))]


def report_engine(engine, age_group, n_groups=None):
    """The report of one engine: the library's kernels on a HIP engine, report_numpy on host views otherwise.  Generations
    are resolved to the engine's day + 1 first; a state deeper than that (only a synthetic one can be) is reported again with
    every chain resolved (reports.with_deep_pass)."""
    _check_unsharded(engine.config)
    if _eng.is_device(engine):
        return _device_reports([engine], None, age_group, n_groups)[0]
    nr_ages = engine.config.nr_ages
    table, ng = _group_table(age_group, nr_ages)
    hot, inf, cnt, counters = _rep.host_state(engine)
    age_start = np.asarray(engine.config.age_start, dtype=np.int64)
    take = lambda depth: report_numpy(hot, inf, cnt, age_start, table[:nr_ages], depth or _rep.day_depth(counters)).words[None]
    return TransmissionReport(_rep.with_deep_pass(take, _UNCONVERGED, engine.config.n_agents)[0], max(ng, int(n_groups or 0)))


def report_group(group, age_group, n_groups=None):
    """The reports of every member of an engine group: one launch per pass on the device, report_engine per member
    otherwise."""
    if not _eng.is_device(group.engines[0]):
        return [report_engine(e, age_group, n_groups) for e in group.engines]
    return _device_reports(group.engines, group, age_group, n_groups)


def report_from_snapshot(snap, age_counts, age_group=None):
    """The report of the state a snapshot holds (snapshot.Snapshot, on the host or the device), from its base records alone.
    age_counts: the population's agents by age (the image's age hash is checked against it); age_group: group of each age
    (default: 10-year bins, 80+)."""
    from . import snapshot as _snap
    img = snap.image if isinstance(snap.image, np.ndarray) else snap.image.cpu().numpy()
    words = np.ascontiguousarray(img).view(np.uint32)
    h = _snap.parse_header(words)
    ages = np.asarray(age_counts, dtype=np.int64)
    age_start = np.zeros(_eng.MAX_AGES + 1, dtype=np.int64)
    age_start[1:len(ages) + 1] = np.cumsum(ages)
    age_start[len(ages) + 1:] = ages.sum()
    if h['magic'] != _snap.MAGIC or h['version'] != _snap.SNAPSHOT_VERSION:
        raise ValueError('not a snapshot image of format version %d' % _snap.SNAPSHOT_VERSION)
    if h['n_agents'] != int(ages.sum()) or h['nr_ages'] != len(ages) \
            or h['ages_hash'] != _snap.fnv1a64(age_start.astype(np.int32).tobytes()):
        raise ValueError('snapshot of another population')
    n = h['n_agents']
    lay = _snap.layout(n, h['n_base'], h['n_slot'], h['qlen'])
    base = words[lay['rb']:lay['rs']].reshape(-1, _snap.RECORD_WORDS)
    rec = (base[:, 0] & 0x7FFFFFFF).astype(np.int64)
    hot = np.zeros(n, dtype=np.uint32)
    inf = np.full(n, -1, dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    hot[rec] = base[:, 1]
    inf[rec] = base[:, 2].view(np.int32)
    cnt[rec] = base[:, 3].view(np.int32)
    table = default_age_groups(len(ages))[0] if age_group is None else age_group
    table, ng = _group_table(table, len(ages))
    counters = words[_snap.HEADER_WORDS:_snap.HEADER_WORDS + _eng.COUNTER_WORDS]
    take = lambda depth: report_numpy(hot, inf, cnt, age_start, table[:len(ages)], depth or _rep.day_depth(counters)).words[None]
    return TransmissionReport(_rep.with_deep_pass(take, _UNCONVERGED, n)[0], ng)


class TransmissionReport(_rep.Report):
    """One report: the words of include/reina_transmission.h as named arrays, plus the statistics derived from them."""
    SCALARS, SCALAR_NAMES = SCALARS, SCALAR_NAMES

    def __init__(self, words, n_groups=MAX_GROUPS, group_labels=None):
        w = self._take(words, REPORT_WORDS, 'a transmission report has %d words' % REPORT_WORDS, n_groups, group_labels)
        self.offspring = w[OFFSPRING:OFFSPRING_SUM].reshape(VARIANTS, SEVERITIES, OUTCOMES, 2, BINS)
        self.offspring_sum = w[OFFSPRING_SUM:OFFSPRING_SUMSQ].reshape(VARIANTS, OUTCOMES)
        self.offspring_sumsq = w[OFFSPRING_SUMSQ:MATRIX].reshape(VARIANTS, OUTCOMES)
        self.matrix = w[MATRIX:GENERATION].reshape(VARIANTS, MAX_GROUPS, MAX_GROUPS)
        self.generations = w[GENERATION:CLUSTERS].reshape(VARIANTS, GENERATIONS)
        self.clusters = w[CLUSTERS:CLUSTER_AGENTS]
        self.cluster_agents = w[CLUSTER_AGENTS:SCALARS]

    def __repr__(self):
        return 'TransmissionReport(infected=%d, roots=%d, linked=%d, max_generation=%d, largest_cluster=%d)' % (
            self.n_infected_agents, self.n_roots, self.n_linked, self.max_generation, self.largest_cluster)

    # ---- offspring statistics: over the agents of `outcome` (default 1: removed and counted into R, the agents whose
    # transmission is over), of one variant or all
    def _sel(self, variant, outcome):
        vs = slice(None) if variant is None else slice(int(variant), int(variant) + 1)
        os_ = slice(None) if outcome is None else slice(int(outcome), int(outcome) + 1)
        hist = self.offspring[vs, :, os_].reshape(-1, BINS).sum(axis=0, dtype=np.uint64)
        return hist, int(self.offspring_sum[vs, os_].sum(dtype=np.uint64)), int(self.offspring_sumsq[vs, os_].sum(dtype=np.uint64))

    def offspring_histogram(self, variant=None, outcome=1):
        return self._sel(variant, outcome)[0]

    def mean_offspring(self, variant=None, outcome=1):
        hist, s, _ = self._sel(variant, outcome)
        n = int(hist.sum())
        return s / n if n else None

    def offspring_variance(self, variant=None, outcome=1):
        """population variance of n_infected (exact sums)"""
        hist, s, q = self._sel(variant, outcome)
        n = int(hist.sum())
        return (q * n - s * s) / (n * n) if n else None

    def dispersion_k(self, variant=None, outcome=1):
        """negative-binomial dispersion by the method of moments, mean^2 / (var - mean); None when var <= mean"""
        m, var = self.mean_offspring(variant, outcome), self.offspring_variance(variant, outcome)
        if m is None or var is None or var <= m:
            return None
        return m * m / (var - m)

    def top_share(self, p=0.2, variant=None, outcome=1):
        """share of the infections caused by the fraction p of the agents that infected the most; exact while the cut lies
        below bin 63 (inside bin 63 its agents are taken as equal)"""
        hist, s, _ = self._sel(variant, outcome)
        n = int(hist.sum())
        if not n or not s:
            return None
        per_bin = [float(b * int(hist[b])) for b in range(BINS - 1)]
        per_bin.append(float(s - sum(b * int(hist[b]) for b in range(BINS - 1))))
        take, got = float(p) * n, 0.0
        for b in range(BINS - 1, -1, -1):
            h = int(hist[b])
            if not h:
                continue
            k = min(take, h)
            got += per_bin[b] * k / h
            take -= k
            if take <= 0:
                break
        return got / s

    def matrix_frame(self, variant=None):
        """linked agents by infector's age group (rows) and own age group (columns), as a pandas DataFrame"""
        import pandas as pd
        m = self.matrix if variant is None else self.matrix[int(variant):int(variant) + 1]
        m = m.sum(axis=0, dtype=np.uint64)[:self.n_groups, :self.n_groups].astype(np.int64)
        labels = self._groups()
        return pd.DataFrame(m, index=pd.Index(labels, name='infector'), columns=pd.Index(labels, name='infectee'))

    def to_dict(self):
        """JSON-able (no pickle): the words as decimal strings of uint64, the groups"""
        return dict(format=TX_VERSION, words=[int(x) for x in self.words], n_groups=self.n_groups, group_labels=self.group_labels)

    @classmethod
    def from_dict(cls, d):
        if d.get('format') != TX_VERSION:
            raise ValueError('transmission report of format %r, this module reads %d' % (d.get('format'), TX_VERSION))
        return cls(np.array([int(x) for x in d['words']], dtype=np.uint64), d['n_groups'], d.get('group_labels'))
