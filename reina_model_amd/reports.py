"""What the tree, log and lineage reports share on the Python side (transmission.py, txlog.py, lineage.py): the counterpart of
csrc/k_addons.inc.  One classification of the links, one age lookup, one forest, one view of an engine's state, one two-pass
rule, one device call, one guard for missing entry points and one base for the Report classes -- so that the three
specifications agree by construction on what a root, a link and a bad link are, as the three kernels do.

And how a report of a log is TAKEN (txlog.py, lineage.py, course.py, vaccination.py, detection.py): each of those modules declares a Kind,
and the three routes -- of one log (report_of), of the members of a log on the device (reports_of_device), of a list of
Contexts (reports_of_contexts) -- and the rule of which group log a list of Contexts shares (group_log, shared_log) are
written here once.

Imports engine only; the report modules import this one, never the other way round.
"""
import collections
import ctypes

import numpy as np

from . import engine as _eng

MAX_GROUPS = 16
NO_ROOT = (1 << 64) - 1        # the largest_root word of a state without a tree (-1 on a Report)
_ROOTED = 1 << 31
_DIST_MAX = (1 << 31) - 1
_MARK = 0xFFFFFFFF

Links = collections.namedtuple('Links', 'state idx s root linked bad')


def links(hot, infector):
    """The classification of every infected agent's link (k_addons.inc: load_links).  state: hot & 7 of every agent; idx: the
    infected agents (state != 0); over idx: s the infector word, root (s == -1), linked (s another agent, in range and
    infected) and bad (neither: the agent heads a tree of its own)."""
    hot = np.asarray(hot).view(np.uint32).ravel()
    state = hot & 7
    idx = np.flatnonzero(state != 0)
    s = np.asarray(infector).view(np.int32).ravel().astype(np.int64)[idx]
    root = s == -1
    in_range = (s >= 0) & (s < len(hot)) & (s != idx)
    linked = np.zeros(len(idx), dtype=bool)
    linked[in_range] = state[s[in_range]] != 0
    return Links(state, idx, s, root, linked, ~root & ~linked)


def default_age_groups(nr_ages):
    """10-year bins, 80+ (what the default population's report groups are)"""
    g = np.minimum(np.arange(_eng.MAX_AGES) // 10, 8)
    return g.astype(np.uint8), ['%d-%d' % (10 * k, 10 * k + 9) for k in range(8)] + ['80+']


def _group_table(age_group, nr_ages):
    """(uint8[MAX_AGES] table, n_groups) from a per-age sequence (ages beyond it: group 0)"""
    g = np.asarray(age_group, dtype=np.int64).ravel()
    if len(g) < nr_ages:
        raise ValueError('age_group: %d ages given, the population has %d' % (len(g), nr_ages))
    g = g[:nr_ages]
    if len(g) and (g.min() < 0 or g.max() >= MAX_GROUPS):
        raise ValueError('age groups are 0 .. %d' % (MAX_GROUPS - 1))
    table = np.zeros(_eng.MAX_AGES, dtype=np.uint8)
    table[:nr_ages] = g
    return table, int(g.max()) + 1 if len(g) else 1


def age_lookup(age_start, age_group):
    """(table, n_groups, nr_ages, age_of) of a specification's age arguments.  age_start: first agent of each age ([A] = N,
    padded with N); age_group: group of each age; age_of(i): the ages of an array of agents (k_common.inc: age_of)."""
    starts = np.asarray(age_start, dtype=np.int64).ravel()
    nr_ages = min(len(np.asarray(age_group).ravel()), _eng.MAX_AGES, len(starts) - 1)
    table, n_groups = _group_table(age_group, nr_ages)
    starts = starts[:nr_ages + 1]
    return table, n_groups, nr_ages, lambda i: np.clip(np.searchsorted(starts, i, side='right') - 1, 0, nr_ages - 1)


def rounds_for(max_depth):
    """pointer-jumping rounds that resolve every generation up to max_depth: ceil(log2(max_depth + 1))"""
    r = 0
    while (1 << r) < int(max_depth) + 1:
        r += 1
    return r


def _jump(parent, dist, rounds):
    """rounds of double-buffered pointer jumping, as k_tx_jump runs them"""
    n = len(parent)
    for _ in range(rounds):
        go = (parent < n) & ((dist & _ROOTED) == 0)
        p = np.where(go, parent, 0).astype(np.int64)
        qp, qd = parent[p], dist[p]
        s = np.minimum((dist & _DIST_MAX).astype(np.int64) + (qd & _DIST_MAX).astype(np.int64), _DIST_MAX).astype(np.uint32)
        parent = np.where(go, qp, parent)
        dist = np.where(go, s | (qd & _ROOTED), dist)
    return parent, dist


def forest(n, idx, s, linked, rounds):
    """(root, generation, conv) over idx after `rounds` of pointer jumping from the links (the parent / dist words k_tx_links and
    k_lineage_links write and k_tx_jump jumps): conv marks the agents whose root was reached; the other two hold only where it does."""
    parent = np.full(n, _MARK, dtype=np.uint32)
    dist = np.zeros(n, dtype=np.uint32)
    parent[idx] = np.where(linked, s, idx).astype(np.uint32)
    dist[idx] = np.where(linked, 1, _ROOTED).astype(np.uint32)
    parent, dist = _jump(parent, dist, rounds)
    return parent[idx].astype(np.int64), (dist[idx] & _DIST_MAX).astype(np.int64), (dist[idx] & _ROOTED) != 0


def largest(heads, sizes):
    """(size, root, key) of the largest tree, the smallest index on ties (k_tx_clusters and k_lineage_roots: the 64-bit atomic
    max of size << 32 | ~root); (0, NO_ROOT, 0) without a tree"""
    if not len(heads):
        return 0, NO_ROOT, 0
    big = int(sizes.max())
    r0 = int(heads[sizes == big][0])
    return big, r0, big << 32 | (~r0 & 0xFFFFFFFF)


def host_state(engine):
    """(hot uint32[N], infector, n_infected, counters) of an engine as host arrays: views of a host-memory engine's buffers,
    copies of a device engine's"""
    host = lambda t: np.asarray(t.cpu().numpy() if hasattr(t, 'cpu') else t)
    cold = host(engine.tensors['cold']).view(np.uint32).reshape(engine.config.n_agents, _eng.COLD_WORDS)
    return host(engine.tensors['hot']).view(np.uint32), cold[:, 2], cold[:, 3], host(engine.tensors['counters'])


def day_depth(counters):
    """the max_depth of a report's first pass: the counter block's day + 1 (no chain of a simulated state is deeper)"""
    day = int(np.asarray(counters).view(np.int32)[_eng.C_NR * _eng.MAX_AGES + _eng.S_DAY])
    return min(max(day, 0), _eng.MAX_DAYS) + 1


def with_deep_pass(take, unconverged_index, n_agents):
    """The two-pass rule.  take(max_depth) -> uint64[members, words]; take(None) resolves generations to the engine's day + 1.
    Members that pass leaves with unconverged agents (only a synthetic state can be that deep) are taken again with every
    chain resolved.  A group is taken again as a group -- one launch per pass, as lineage.report_group always did -- and only
    the unconverged members' rows are replaced: the others keep the words of their first pass."""
    w = take(None)
    deep = np.flatnonzero(w[:, unconverged_index])
    if len(deep):
        w[deep] = take(n_agents)[deep]
    return w


def member_rows(w):
    """the rows of uint64[members, words], each an array of its own (a member's report does not keep the whole group's block
    alive); the one row of a single engine is handed on as it is"""
    return [w[0]] if len(w) == 1 else [r.copy() for r in w]


def entry_points(engine, attr, what, header):
    """engine.<attr>: the entry points of one of the headers beside reina_hip.h, EngineError when the library has none"""
    f = getattr(engine, attr, None)
    if f is None:
        raise _eng.EngineError('the engine library has no %s entry points (include/%s)' % (what, header))
    return f


def device_words(engine, f, name, head, members, words, scratch_bytes=None, stale=(), group=False):
    """uint64[members, words] of one launch of the report entry point f[name](*head, [scratch,] report, stream).  scratch:
    scratch_bytes per member (the members of a group share one population, so one size), as an array of pointers for a `group`
    entry point -- one member or many -- and one pointer otherwise.  `stale`: the engines the launch ran on behind their backs."""
    torch, dev = engine.alloc.torch, engine.alloc.device
    scratch = [torch.empty(scratch_bytes, dtype=torch.uint8, device=dev) for _ in range(members if scratch_bytes else 0)]
    rep = torch.empty(members * words, dtype=torch.int64, device=dev)
    ptrs = [s.data_ptr() for s in scratch]
    if scratch:
        head = tuple(head) + ((ctypes.c_void_p * members)(*ptrs) if group else ptrs[0],)
    engine._check(f[name](*head, rep.data_ptr(), engine.alloc.stream()), name)
    _eng.mark_stale(stale)
    return rep.cpu().numpy().view(np.uint64).reshape(members, words)   # (the copy waits for the launch: the scratch may go)


# ------------------------------------------------------------------------------------------------ taking a report of a log

# What is particular to one report taken of a log; its module declares one (txlog.LOG, lineage.LINEAGE, course.COURSE,
# vaccination.VACCINATION, detection.DETECTION) and binds its public names onto the three routes below.
#   name         the report's name in refusals ('log_reports')
#   of           what it is taken of: the Context attribute that holds the log ('transmission_log' or 'course_log')
#   arguments    (ctx, *args) -> (table, labels, *params): the Context's report groups and the report's own parameters, checked
#   numpy        (ctx, log, table, params) -> take(max_depth) -> uint64[words]: the specification on host copies
#   report       the Report class: report(words, *params, n_groups, labels, start_date, *extra)
#   words        (*params) -> the words of one report
#   names        the entry points of one engine's log and of a group's (the same twice where the library has one for both)
#   on           (DeviceLog of a group) -> what of it the entry points take: the log itself, or its course
#   entry        None: the entry points are those of what it is taken of (there whenever that is on the device); or
#                (engine attribute, what, header) of entry points of its own, which a library may lack
#   scratch      (n_agents) -> scratch bytes per member, None without scratch
#   unconverged  the index of the word that asks for the deep pass (with_deep_pass: max_depth follows the params); None without
#   extra        (ctx, table) -> further arguments of `report`, the same for every member
#   arrays       how many of the LAST params are host arrays with one row per member (the regime report's labels): the entry
#                point takes each as a pointer behind the integer params, `report` and `numpy` get a member's own row
Kind = collections.namedtuple('Kind', 'name of arguments numpy report words names on entry scratch unconverged extra arrays',
                              defaults=(lambda glog: glog, None, None, None, None, 0))


def group_log(contexts):
    """the txlog.DeviceLog these Contexts share when they are the whole of one logged group, in member order; None otherwise"""
    logs = [getattr(c, 'transmission_log', None) for c in contexts]
    glog = logs[0].device if logs and logs[0] is not None else None
    if glog is not None and glog.group is not None and all(t is not None and t.device is glog for t in logs) \
            and [t.member for t in logs] == list(range(glog.members)):
        return glog
    return None


def shared_log(contexts, group, refusal):
    """The group log of Contexts about to be run or cloned as `group`: None when none of them keeps a transmission log, the
    group's txlog.DeviceLog when they are the whole of that logged group (group_log), ValueError(refusal) otherwise -- logs
    kept by some only, logs of their own, or of another group."""
    if not any(getattr(c, 'transmission_log', None) is not None for c in contexts):
        return None
    glog = group_log(contexts)
    if glog is None or glog.group is not group:
        raise ValueError(refusal)
    return glog


def _launches(kind, dev):
    """may the library take this kind of report of `dev` (what a log keeps on the device, or None)"""
    return dev is not None and (kind.entry is None or getattr(dev.engine, kind.entry[0], None) is not None)


def _taken(kind, take, n_agents):
    return take(None) if kind.unconverged is None else with_deep_pass(take, kind.unconverged, n_agents)


def _split(kind, params):
    """(the integer params, the arrays by member) of a kind's params"""
    params = tuple(params)
    cut = len(params) - kind.arrays
    return params[:cut], params[cut:]


def _member_params(kind, params, m):
    """the params as member m's report takes them: of every array its own row"""
    ints, arrays = _split(kind, params)
    return ints + tuple(a[m] for a in arrays)


def _made(kind, w, contexts, table, labels, params):
    extra = kind.extra(contexts[0], table) if kind.extra is not None else ()
    return [kind.report(r, *_member_params(kind, params, m), len(labels), labels, c.start_date, *extra)
            for m, (r, c) in enumerate(zip(member_rows(w), contexts))]


def device_take(kind, dev, table, n_groups, params):
    """take(max_depth) -> uint64[members, words] of `dev`, a txlog.DeviceLog or course.DeviceCourse: one launch for all members"""
    e = dev.engine
    f = dev.f if kind.entry is None else entry_points(e, *kind.entry)
    group = dev.group is not None
    depth = (lambda d: (int(d or 0),)) if kind.unconverged is not None else (lambda d: ())
    ints, arrays = _split(kind, params)
    arrays = [np.ascontiguousarray(a) for a in arrays]   # (alive as long as the callable: the entry point reads them where they are)
    if any(len(a) != dev.members for a in arrays):
        raise ValueError('%s: one row per member is wanted' % kind.name)
    return lambda d=None: device_words(
        e, f, kind.names[group], (dev._h, table.ctypes.data, int(n_groups)) + tuple(int(p) for p in ints) + depth(d) +
        tuple(ctypes.c_void_p(a.ctypes.data) for a in arrays), dev.members,
        kind.words(*params), kind.scratch(e.config.n_agents) if kind.scratch is not None else None, dev.engines, group)


def reports_of_device(kind, dev, contexts, *args):
    """The reports of the members of `dev` (of a logged group, or of the one engine of a log on the device): one launch for all
    members, one per pass for a kind that takes the deep pass.  The arguments are checked before `dev` is asked for anything."""
    c0 = contexts[0]
    table, labels, *params = kind.arguments(c0, *args)
    t8, ng = _group_table(table, c0.nr_ages)
    w = _taken(kind, device_take(kind, dev, t8, max(ng, len(labels)), params), c0.engine.config.n_agents)
    return _made(kind, w, contexts, table, labels, params)


def report_of(kind, log, *args):
    """The report of one log (a Context's TransmissionLog or CourseLog): the library's kernels when the log is a single engine's
    on the device and the kind's entry points are there, the specification on host copies otherwise -- oracle B, a log kept in
    host memory, a member of a group taken on its own."""
    ctx, dev = log.ctx, log.device
    if _launches(kind, dev) and dev.group is None:
        return reports_of_device(kind, dev, [ctx], *args)[0]
    table, labels, *params = kind.arguments(ctx, *args)
    take = kind.numpy(ctx, log, table, _member_params(kind, params, 0))
    w = _taken(kind, lambda depth: take(depth)[None], ctx.engine.config.n_agents)
    return _made(kind, w, [ctx], table, labels, params)[0]


def reports_of_contexts(kind, contexts, *args):
    """The reports of a list of Contexts, between the same two days: reports_of_device when they are the whole of one logged
    group in member order and the library can take the kind of it, report_of one by one otherwise."""
    contexts = list(contexts)
    if any(getattr(c, kind.of) is None for c in contexts):
        raise ValueError('%s: a context keeps no %s' % (kind.name, kind.of.replace('_', ' ')))
    glog = group_log(contexts)
    dev = kind.on(glog) if glog is not None else None
    if _launches(kind, dev) and all(getattr(c, kind.of).device is dev for c in contexts):
        return reports_of_device(kind, dev, contexts, *args)
    return [report_of(kind, getattr(c, kind.of), *args) for c in contexts]


class Report:
    """What the three Report classes share: the words, the groups, the scalars by name and equality.  A subclass names its
    SCALARS offset and SCALAR_NAMES, and in IDENTITY the parameters that belong to its identity beside the words."""
    SCALARS, SCALAR_NAMES, IDENTITY = 0, (), ()

    def _take(self, words, count, message, n_groups, group_labels):
        w = np.asarray(words, dtype=np.uint64).ravel()
        if len(w) != count:
            raise ValueError(message)
        self.words, self.n_groups = w, int(n_groups)
        self.group_labels = list(group_labels) if group_labels is not None else None
        for k, name in enumerate(self.SCALAR_NAMES):
            setattr(self, name, int(w[self.SCALARS + k]))
        if getattr(self, 'largest_root', None) == NO_ROOT:
            self.largest_root = -1
        return w

    def _groups(self):
        return self.group_labels or [str(k) for k in range(self.n_groups)]

    def _dates(self):
        """the index of a table by day (reports with n_days and start_date): dates from start_date, day numbers without one"""
        import pandas as pd
        if self.start_date is None:
            return pd.RangeIndex(self.n_days, name='day')
        return pd.date_range(str(self.start_date), periods=self.n_days, name='date')

    def __eq__(self, other):
        return isinstance(other, type(self)) and all(getattr(self, k) == getattr(other, k) for k in self.IDENTITY) \
            and np.array_equal(self.words, other.words)
