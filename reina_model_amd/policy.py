"""Triggered interventions: policies that react to a run's own counters (include/reina_policy.h).

Every other intervention is dated.  A `Policy` is a ladder of levels; each level is a list of UNDATED `limit-mobility` /
`wear-masks` interventions in force while the level is; a rule moves a run up and down the ladder from one of its counters.
On the GPU the decision and the table switch are one kernel queued ahead of every day (`k_policy`), per member of an engine
group, and the run keeps its single wait at the end.  This module is the definition:

SIGNAL   x_now(d) = the sum over the 128 words of one per-age counter row (engine.C_NAMES) of the counter block BEFORE day d's
         opening -- the values history row d holds, what generate_state() shows on that date.  kind 'level': x(d) = x_now(d);
         'increment' over n days (1..28): x(d) = x_now(d) - x_now(max(d - n, first)), `first` = the first day of the unbroken
         sequence of days the policy has seen (the last 32 daily values are kept in a ring; a day that does not follow the
         last one seen starts a new sequence).  Integers throughout.
RULE     L levels (2..8), `up[0..L-2]` non-decreasing, `down[j] <= up[j]`, `review_every` >= 1, `min_days` >= 0, `start` (a
         date; default the scenario's start date).  A run starts at level 0.  On a review day (d >= start and
         (d - start) % review_every == 0), with l the current level: escalate to the highest j > l with x >= up[j - 1], if
         any (jumps allowed); otherwise, if l > 0, x < down[l - 1] and level l has governed at least `min_days` days, relax
         to l - 1.  The level decided before day d's opening governs day d.
TABLES   For every stretch of unchanged dated tables (a plan segment; a run that begins between two dated changes begins
         with one) and every level l: a copy of the ContactMatrix as the dated schedule left it at the stretch's upload, with
         level l's interventions applied in list order exactly as Context.apply_intervention applies them, rebuilt and packed
         by Context._packed_tables.  Level 0 is the dated upload, byte for byte.  Mask shares take effect only when tables
         are uploaded: a level's tables carry the mask shares of the stretch's upload with the level's wear-masks applied.
         On a day that starts a stretch the dated interventions come first, then the rule, then the run takes its level's
         tables of the new stretch.
TRACE    `policy_levels[d]`: the level in force on day d.  `mobility_history[d]`, the reference's mobility factor column, is
         what generate_state() BEFORE day d would report: the value of (stretch, level) of day d - 1 -- the mobility factor
         the last limit-mobility applied left, dated or the level's -- and on a run's first day the value the Context carried.

Only interventions that act through the contact tables can be triggered: testing modes, capacity, imports and vaccination
travel in the day descriptor, which the members of a group share.

`step_numpy` is the executable specification of the rule; `run_host_driven` is the plain formulation of a policy run (read the
counters, decide, upload, iterate: one host round trip a day) that works on any engine and is what the device path is tested
against.
"""
import copy
import ctypes
from datetime import date

import numpy as np

from . import engine as _eng
from .dayrun import History, replay_plan, stream_days

POLICY_VERSION = 1
MAX_LEVELS = 8
RING = 32
TRACE_WORDS = 2
KINDS = ('level', 'increment')
TRIGGERABLE = ('limit-mobility', 'wear-masks')
POLICY_FUNCTIONS = ('policy_version', 'policy_create', 'group_policy_create', 'policy_destroy', 'policy_upload_level',
                    'policy_run_days', 'group_policy_run_days', 'policy_read_trace')


class RuleABI(ctypes.Structure):
    _fields_ = [('n_levels', ctypes.c_uint32), ('signal', ctypes.c_uint32), ('kind', ctypes.c_uint32),
                ('n_days', ctypes.c_uint32), ('review_every', ctypes.c_uint32), ('min_days', ctypes.c_uint32),
                ('start_day', ctypes.c_uint32), ('reserved_', ctypes.c_uint32),
                ('up', ctypes.c_int32 * MAX_LEVELS), ('down', ctypes.c_int32 * MAX_LEVELS)]
_vp, _u32 = ctypes.c_void_p, ctypes.c_uint32
_POLICY_ARGTYPES = {'policy_create': [_vp, ctypes.POINTER(RuleABI), ctypes.POINTER(_vp)],
                    'group_policy_create': [_vp, ctypes.POINTER(RuleABI), ctypes.POINTER(_vp)],
                    'policy_destroy': [_vp], 'policy_upload_level': [_vp, _u32, ctypes.POINTER(_eng.ContactTablesABI), _vp],
                    'policy_run_days': [_vp, ctypes.POINTER(_eng.Day), _u32, _vp, _vp],
                    'group_policy_run_days': [_vp, ctypes.POINTER(_eng.Day), _u32, ctypes.POINTER(_vp), _vp],
                    'policy_read_trace': [_vp, _u32, _u32, _vp, _vp]}


def bind_policy_abi(lib, prefix):
    """The policy entry points of a library, or None when it has none (the CPU checker's)."""
    return _eng.bind_optional_abi(lib, prefix, POLICY_FUNCTIONS, _POLICY_ARGTYPES, 'policy_version', POLICY_VERSION)


class Signal:
    """One per-age counter row (engine.C_NAMES), summed over the ages: the sum itself (kind 'level') or its increment over
    `days` days (kind 'increment', 1 <= days <= 28)."""

    def __init__(self, counter, kind='level', days=7):
        if counter not in _eng.C_NAMES:
            raise ValueError('Signal.counter: %r is not a per-age counter (%s)' % (counter, ', '.join(_eng.C_NAMES)))
        if kind not in KINDS:
            raise ValueError("Signal.kind: %r is neither 'level' nor 'increment'" % (kind,))
        if kind == 'increment' and not (isinstance(days, (int, np.integer)) and 1 <= int(days) <= 28):
            raise ValueError('Signal.days: an increment is taken over 1..28 days, not %r' % (days,))
        self.counter = counter
        self.kind = kind
        self.days = int(days) if kind == 'increment' else 0
        self.row = _eng.C_NAMES.index(counter)


def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


class Policy:
    """signal: a Signal; levels: L lists of undated intervention tuples ([type, value...], as in variables['interventions']
    without the date; level 0 is usually empty); up / down: L - 1 integer thresholds each; review_every, min_days: days;
    start: an ISO date or None (the scenario's start date)."""

    def __init__(self, signal, levels, up, down, review_every=1, min_days=0, start=None):
        if not isinstance(signal, Signal):
            raise ValueError('Policy.signal: a policy.Signal is wanted')
        levels = [[list(iv) for iv in lv] for lv in levels]
        if not 2 <= len(levels) <= MAX_LEVELS:
            raise ValueError('Policy.levels: 2..%d levels, not %d' % (MAX_LEVELS, len(levels)))
        for k, lv in enumerate(levels):
            for iv in lv:
                if not iv or iv[0] not in TRIGGERABLE:
                    raise ValueError('Policy.levels[%d]: only %s can be triggered (they act through the contact tables), not %r'
                                     % (k, ' / '.join(TRIGGERABLE), iv[0] if iv else iv))
        up, down = list(up), list(down)
        if len(up) != len(levels) - 1 or not all(_is_int(x) for x in up):
            raise ValueError('Policy.up: %d integer thresholds are wanted' % (len(levels) - 1))
        if len(down) != len(levels) - 1 or not all(_is_int(x) for x in down):
            raise ValueError('Policy.down: %d integer thresholds are wanted' % (len(levels) - 1))
        if any(abs(int(x)) >= 2 ** 31 for x in up + down):
            raise ValueError('Policy.up / Policy.down: thresholds are 32-bit counts')
        if any(up[j] < up[j - 1] for j in range(1, len(up))):
            raise ValueError('Policy.up: thresholds must be non-decreasing')
        if any(down[j] > up[j] for j in range(len(up))):
            raise ValueError('Policy.down: down[j] <= up[j] is required')
        if not _is_int(review_every) or review_every < 1:
            raise ValueError('Policy.review_every: at least 1')
        if not _is_int(min_days) or min_days < 0:
            raise ValueError('Policy.min_days: at least 0')
        if start is not None:
            try:
                date.fromisoformat(str(start))
            except ValueError:
                raise ValueError('Policy.start: %r is not an ISO date (YYYY-MM-DD)' % (start,)) from None
        self.signal = signal
        self.levels = levels
        self.up = [int(x) for x in up]
        self.down = [int(x) for x in down]
        self.review_every = int(review_every)
        self.min_days = int(min_days)
        self.start = None if start is None else str(start)

    @property
    def n_levels(self):
        return len(self.levels)

    def start_day(self, start_date):
        """the first review day as a day number of a scenario that starts on `start_date`"""
        if self.start is None:
            return 0
        d = (date.fromisoformat(self.start) - date.fromisoformat(str(start_date))).days
        if not 0 <= d < _eng.MAX_DAYS:
            raise ValueError('Policy.start: %s lies outside the %d days from %s' % (self.start, _eng.MAX_DAYS, start_date))
        return d

    def rule_abi(self, start_date):
        r = RuleABI()
        r.n_levels = self.n_levels
        r.signal = self.signal.row
        r.kind = KINDS.index(self.signal.kind)
        r.n_days = self.signal.days
        r.review_every = self.review_every
        r.min_days = self.min_days
        r.start_day = self.start_day(start_date)
        for j in range(self.n_levels - 1):
            r.up[j] = self.up[j]
            r.down[j] = self.down[j]
        return r

    def new_state(self, start_date=None, start_day=None):
        """the state step_numpy advances: level 0, nothing seen"""
        if start_day is None:
            start_day = self.start_day(start_date) if start_date is not None else 0
        return dict(policy=self, start_day=int(start_day), level=0, in_force=0, first_day=0, next_day=0, seen=False,
                    ring=np.zeros(RING, dtype=np.int64), x=0)


def step_numpy(state, counters_row, day):
    """The rule for day `day`: `counters_row` is the counter block [COUNTER_WORDS] before the day's opening (history row
    `day`).  Advances `state` (Policy.new_state) and returns the level that governs the day; state['x'] is the signal."""
    p = state['policy']
    day = int(day)
    row = p.signal.row
    x_now = int(np.asarray(counters_row[row * _eng.MAX_AGES:(row + 1) * _eng.MAX_AGES], dtype=np.int64).sum())
    first = state['first_day'] if state['seen'] and state['next_day'] == day else day
    ring = state['ring']
    x = x_now
    if p.signal.kind == 'increment':
        back = max(day - p.signal.days, first)
        x = x_now - (x_now if back == day else int(ring[back % RING]))
    level, in_force = state['level'], state['in_force']
    start = state['start_day']
    if day >= start and (day - start) % p.review_every == 0:
        to = level
        for j in range(p.n_levels - 1, level, -1):
            if x >= p.up[j - 1]:
                to = j
                break
        if to == level and level > 0 and x < p.down[level - 1] and in_force >= p.min_days:
            to = level - 1
        if to != level:
            level, in_force = to, 0
    ring[day % RING] = x_now
    state.update(level=level, in_force=in_force + 1, first_day=first, next_day=day + 1, seen=True, x=x)
    return level


# ------------------------------------------------------------------------------------------------ the bank

class _MatrixHolder:
    """what Context.apply_intervention / Context._packed_tables touch for limit-mobility and wear-masks"""

    def __init__(self, ctx, matrix):
        self.contact_matrix = matrix
        self.nr_ages = ctx.nr_ages


def build_bank(ctx, policy, mask_base=None):
    """The tables of every level for the stretch that begins at the Context's present contact matrix: a list of L packed
    table tuples (Context._packed_tables) and the L mobility factors generate_state would report.  `mask_base`
    [MAX_AGES, 8] float32: the mask shares of the stretch's dated upload (default: those of the Context's last one).  The
    Context's own matrix is not touched."""
    from .interventions import iv_tuple_to_obj
    from .model import Context
    if mask_base is None:
        mask_base = ctx._uploaded_mask
    cm = ctx.contact_matrix
    vnames = tuple(ctx.variant_names[1:])
    tables, factors = [], []
    for ivs in policy.levels:
        m = copy.copy(cm)
        m.mobility_factors = [list(f) for f in cm.mobility_factors]
        m.mask_probabilities = np.asarray(mask_base, dtype=np.float32)[:ctx.nr_ages, :m.mask_probabilities.shape[1]].astype(np.float64)
        m.mobility_factor_changed = False
        holder = _MatrixHolder(ctx, m)
        for iv in ivs:
            Context.apply_intervention(holder, iv_tuple_to_obj([iv[0], None] + list(iv[1:]), vnames))
        m.generate_contact_probabilities()   # (mask shares reach the tables' own copy only through a rebuild)
        tables.append(Context._packed_tables(holder))
        factors.append(float(m.mobility_factor))
    return tables, factors


def mobility_trace(first_value, segment_of_day, levels, factors):
    """mobility_history of a policy run: day d reports the factor of (stretch, level) of day d - 1, the first day
    `first_value`.  factors[s][l]; segment_of_day, levels: one entry per day."""
    out = [float(first_value)]
    for k in range(1, len(levels)):
        out.append(float(factors[segment_of_day[k - 1]][int(levels[k - 1])]))
    return out[:len(levels)]


def _first_mobility(ctx, dated, day):
    """what a policy run that begins on `day` reports on its first day: the value the Context's last policy run left if this
    run continues it, else the dated one"""
    carried = getattr(ctx, '_policy_mobility', None)
    return carried[1] if carried is not None and carried[0] == day else float(dated)


def level_by_day(ctx):
    """Context.policy_level_by_day: int8[MAX_DAYS], the level of every day the Context has run under a policy, -1 elsewhere"""
    by_day = getattr(ctx, 'policy_level_by_day', None)
    if by_day is None:
        by_day = ctx.policy_level_by_day = np.full(_eng.MAX_DAYS, -1, dtype=np.int8)
    return by_day


def _finish(ctx, first_value, levels, segment_of_day, factors, end_day):
    """the trace of a policy run onto the Context: policy_levels and mobility_history are the run's own days, policy_level_by_day
    accumulates over the runs"""
    levels = np.asarray(levels, dtype=np.int32)
    if len(levels):
        ctx.mobility_history = mobility_trace(first_value, segment_of_day, levels, factors)
        ctx._policy_mobility = (int(end_day), float(factors[segment_of_day[-1]][int(levels[-1])]))
        level_by_day(ctx)[int(end_day) - len(levels):int(end_day)] = levels
    else:
        ctx.mobility_history = []
    ctx.policy_levels = levels


def _note_dated_upload(ctx):
    """a day rebuilt the dated tables: their upload would carry the mask shares as they stand (Context._packed_tables)"""
    ctx._mask_block()


def _end_device_run(ctx, trace, member, start_day, dated_first, segment_of_day, factors):
    """The end of a device run for one Context: `trace` (DevicePolicy.read_trace, the run's wait) of `member` becomes its
    policy_signal, policy_levels and mobility_history.  dated_first: the dated mobility factor before the first day."""
    days = trace.shape[1]
    first_value = _first_mobility(ctx, dated_first, start_day) if days else 0.0
    ctx.policy_signal = trace[member, :, 1].copy()
    _finish(ctx, first_value, trace[member, :, 0], segment_of_day, factors, start_day + days)


def check_capable(ctx):
    if ctx.n_shards != 1 or ctx.always_collective:
        raise ValueError('policy: sharded Contexts are refused (the signal would need the all-reduce of the shards)')


# ------------------------------------------------------------------------------------------------ the plain formulation

def run_host_driven(ctx, policy, days, record_history=True):
    """`days` days under `policy`, the plain way: per day read the counters, step_numpy, upload the level's tables when they
    change, iterate -- one blocking round trip a day, on any engine.  Returns history like Context.run and sets
    ctx.policy_levels / ctx.mobility_history.  The policy's state stays with the Context (ctx._policy_state): further calls
    continue it.  A transmission log the Context keeps in host memory, and its course log, are recorded behind every day
    (txlog.record_numpy / CourseLog.record_host, as txlog.run_host_driven does): the specification of the logged policy run."""
    check_capable(ctx)
    log = ctx.transmission_log
    if log is not None and log.on_device:
        raise ValueError('run_host_driven: this Context keeps its log on the device')
    state = getattr(ctx, '_policy_state', None)
    if state is None or state['policy'] is not policy:
        state = ctx._policy_state = policy.new_state(ctx.start_date)
    hist = History(days, record_history, ctx=ctx)
    levels, seg_of_day, factors = [], [], []
    bank, in_force = None, None
    first_value = _first_mobility(ctx, ctx.contact_matrix.mobility_factor, ctx.day)
    for k in range(days):
        counters = ctx.engine.read_counters()
        level = step_numpy(state, counters, ctx.day)
        d, changed = ctx._build_day(hist.at(k))
        if changed:
            _note_dated_upload(ctx)
        if changed or bank is None:
            bank, f = build_bank(ctx, policy)
            factors.append(f)
            in_force = None
        if in_force != level:
            ctx.engine.upload_contact_tables(*bank[level])
            in_force = level
        ctx.engine.step_day(d)
        ctx.day += 1
        if log is not None:
            log.record_day(d.day)
        levels.append(level)
        seg_of_day.append(len(factors) - 1)
    _finish(ctx, first_value, levels, seg_of_day, factors, ctx.day)
    return _history_or_wait(ctx, hist)


def _history_or_wait(ctx, hist):
    """a policy run ends with a wait either way: for its history, or (record_history=False) for the counters"""
    if hist.buf is None:
        ctx.synchronize()
    return hist.to_host()


# ------------------------------------------------------------------------------------------------ the device route

class DevicePolicy(_eng.Handle):
    """A policy on the device for one engine or one engine group (include/reina_policy.h)."""
    DESTROY = 'policy_destroy'

    def __init__(self, policy, start_date, engine=None, group=None):
        owner = engine if engine is not None else group.engines[0]
        self.f = owner.policy_f
        if self.f is None:
            raise _eng.EngineError('this engine library has no policy entry points: use policy.run_host_driven')
        self.owner = owner
        self.alloc = owner.alloc
        self.group = group
        self.members = 1 if group is None else len(group.engines)
        self._grouped = group is not None
        self._h = ctypes.c_void_p()
        rule = policy.rule_abi(start_date)
        if group is None:
            owner._check(self.f['policy_create'](owner._h, ctypes.byref(rule), ctypes.byref(self._h)), 'policy_create')
        else:
            owner._check(self.f['group_policy_create'](group._h, ctypes.byref(rule), ctypes.byref(self._h)), 'group_policy_create')
        self.policy = policy
        self.log = None   # the txlog.DeviceLog of the same engine / group, when its days are to be recorded (run_day_array)

    def upload_bank(self, tables):
        for level, tab in enumerate(tables):
            t, _keep = _eng.Engine._tables_abi(*tab)
            self.owner._check(self.f['policy_upload_level'](self._h, level, ctypes.byref(t), self.alloc.stream()), 'policy_upload_level')

    def run_day_array(self, arr, n, history):
        """history: a device pointer (one engine) or one per member (a group), or None.  With a device log (self.log): the
        combined entry points of include/reina_regime.h, the log's record launch behind every day."""
        f, head, tail = self.f, (self._h,), 'policy_run_days'
        if self.log is not None:
            f = _regime_entry_points(self.owner)
            head, tail = (self._h, self.log._h), 'policy_txlog_run_days'
        if self._grouped:
            hp = _eng.member_pointers(self.group.engines, history)
            self.owner._check(f['group_' + tail](*head, arr, n, hp, self.alloc.stream()), 'group_' + tail)
        else:
            if self.log is not None:
                self.log._touch()
            self.owner._check(f[tail](*head, arr, n, history, self.alloc.stream()), tail)

    def read_trace(self, first_day, days):
        """[members, days, 2] (level in force, signal); waits for the stream"""
        out = np.zeros((self.members, max(days, 0), TRACE_WORDS), dtype=np.int32)
        self.owner._check(self.f['policy_read_trace'](self._h, int(first_day), int(days), out.ctypes.data, self.alloc.stream()), 'policy_read_trace')
        return out


def plan_segments_of_days(plan):
    out = []
    for si, (_, _, n) in enumerate(plan['segments']):
        out += [si] * n
    return out


def _regime_entry_points(engine):
    from . import reports as _rep
    return _rep.entry_points(engine, 'regime_f', 'policy-and-log', 'reina_regime.h')


def _device_of(ctx):
    """the Context's DevicePolicy, recording into the Context's own device log when it keeps one (a log in host memory, or a
    group's, cannot follow the device route)"""
    log = ctx.transmission_log
    if log is not None and (log.device is None or log.device.group is not None):
        raise ValueError('policy: this Context keeps its log %s: the device route cannot record it'
                         % ('in host memory (policy.run_host_driven runs its days)' if log.device is None else "with its group's"))
    dev = getattr(ctx, '_policy_device', None)
    if dev is None or dev.policy is not ctx.policy:
        dev = ctx._policy_device = DevicePolicy(ctx.policy, ctx.start_date, engine=ctx.engine)
    dev.log = None if log is None else log.device
    return dev


def run_device(ctx, days, record_history=True):
    """Context.run for a Context with a policy attached: day descriptors are built on the host and handed to the library in
    growing chunks (dayrun.stream_days), k_policy ahead of every day, a bank of level tables at every stretch of dated tables
    and on the run's first day; one wait at the end, which brings the trace back with the history."""
    check_capable(ctx)
    dev, policy = _device_of(ctx), ctx.policy
    hist = History(days, record_history, ctx=ctx)
    start_day = ctx.day
    seg_of_day, factors = [], []

    def on_day(d, changed):
        upload = None
        if changed:
            _note_dated_upload(ctx)
        if changed or not factors:
            bank, f = build_bank(ctx, policy)
            factors.append(f)
            upload = lambda: dev.upload_bank(bank)
        seg_of_day.append(len(factors) - 1)
        return upload

    dated = stream_days(ctx, days, dev, hist, on_day)
    _end_device_run(ctx, dev.read_trace(start_day, days), 0, start_day, dated[0] if days else 0.0, seg_of_day, factors)
    return _history_or_wait(ctx, hist)


def run_plan_device(ctx, plan, record_history=True):
    """Context.run_plan for a Context with a policy attached: the plan's days with k_policy ahead of each, one wait at the end"""
    banks = plan.get('policy_banks')
    if banks is None or plan.get('policy') is not ctx.policy:
        raise ValueError('run_plan: this Context carries a policy; the plan must be made with it (make_plan(days, policy=...))')
    dev = _device_of(ctx)
    days, start_day = plan['days'], plan['start_day']
    hist = History(days, record_history, ctx=ctx)
    replay_plan(plan, dev, hist, lambda si, tables: dev.upload_bank(banks[si][0]))
    ctx.day = start_day + days
    _end_device_run(ctx, dev.read_trace(start_day, days), 0, start_day, plan['mobility_history'][0] if days else 0.0,
                    plan_segments_of_days(plan), [b[1] for b in banks])
    return _history_or_wait(ctx, hist)
