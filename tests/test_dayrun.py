"""The calls the library sees (reina_model_amd/dayrun.py): every way a Context runs its days, with the entries of `engine.f`
of oracle-B engines wrapped by recorders -- entry point, n, the history pointer as an offset into its buffer, a checksum of
every table upload -- and, for the device routes oracle B has no entry points for (policy, transmission log), recording
stand-ins that forward their days to run_days_hist / group_run_days.

The expected traces (tests/test_dayrun_traces.json) were recorded with this very recorder on the commit before the day runner
existed (docs/HISTORY.md section 6 names it): `python tests/test_dayrun.py --record` rewrites the file from the code as it
stands, which is only ever right on a commit whose call order is the one to keep."""
import copy
import ctypes
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]   # (for `python tests/test_dayrun.py --record`)
import par_backend
from policy_util import never_policy
from reina_model_amd import datasets, ensemble, simulation
from reina_model_amd import engine as eng
from reina_model_amd.variables import VARIABLE_DEFAULTS

TRACES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_dayrun_traces.json')
DAYS, AGENTS, SEEDS = 200, 20000, (5, 6, 7)
SKIPPED = ('create', 'destroy', 'bind_buffers', 'last_error', 'abi_version')   # (destroy runs when the collector pleases)
TABLE_BYTES = (4 * eng.MAX_AGES, 4 * eng.MAX_AGES, 4 * eng.MAX_AGES * eng.MAX_ENTRIES, 4 * eng.MAX_AGES * eng.MAX_ENTRIES,
               4 * eng.MAX_AGES * 8)


def _tables_crc(ref):
    t = ref._obj
    crc = zlib.crc32(bytes(memoryview(t))[5 * ctypes.sizeof(ctypes.c_void_p):])
    for name, size in zip(('nr_contacts_by_age', 'count', 'threshold', 'meta', 'mask_p'), TABLE_BYTES):
        crc = zlib.crc32(ctypes.string_at(getattr(t, name), size), crc)
    return crc


class Recorder:
    """one scenario's log: the library calls of all its engines in order, allocations and read-backs among them"""

    def __init__(self):
        self.log = []
        self.bufs = []       # every buffer allocated while recording, kept alive: an address names one buffer
        self.members = {}    # engine / group / attachment handle -> label

    def where(self, p):
        """a device pointer as [buffer number among those allocated since the recording began, byte offset]"""
        if p is None:
            return None
        p = int(p)
        for k, b in enumerate(self.bufs):
            if b.ctypes.data <= p < b.ctypes.data + max(b.nbytes, 1):
                return [k, p - b.ctypes.data]
        return ['?', 0]

    def label(self, h):
        h = h.value if hasattr(h, 'value') else h
        return self.members.get(h, '?')

    def event(self, name, args):
        e = [name]
        if name in ('run_days_hist', 'policy_run_days', 'txlog_run_days'):
            e += [self.label(args[0]), int(args[2]), int(args[1][0].day), self.where(args[3])]
        elif name in ('group_run_days', 'group_policy_run_days', 'group_txlog_run_days'):
            hp = args[3]
            e += [self.label(args[0]), int(args[2]), int(args[1][0].day), None if hp is None else [self.where(p) for p in hp]]
        elif name in ('upload_contact_tables', 'group_upload_contact_tables'):
            e += [self.label(args[0]), _tables_crc(args[1])]
        elif name == 'policy_upload_level':
            e += [self.label(args[0]), int(args[1]), _tables_crc(args[2])]
        elif name == 'read_history':
            e += [self.label(args[0]), self.where(args[1]), int(args[2])]
        elif name == 'policy_read_trace':
            e += [self.label(args[0]), int(args[1]), int(args[2])]
        elif name == 'step_phase':
            e += [self.label(args[0]), int(args[1]._obj.day), int(args[2]), self.where(args[1]._obj.history_row)]
        elif name == 'step_day':
            e += [self.label(args[0]), int(args[1]._obj.day), self.where(args[1]._obj.history_row)]
        elif name in ('read_counters', 'txlog_record_day', 'policy_destroy', 'txlog_destroy', 'group_destroy'):
            e += [self.label(args[0])]
        self.log.append(e)

    def attach(self, ctx, label):
        """wrap the entries of ctx.engine.f and the engine's allocator; give the engine the stand-in attachments"""
        e = ctx.engine
        self.members[e._h.value] = label
        for name in list(e.f):
            if name not in SKIPPED:
                e.f[name] = self._wrap(name, e.f[name])
        a = e.alloc
        for kind in ('zeros', 'empty'):
            setattr(a, kind, self._alloc(kind, getattr(a, kind)))
        to_host = a.to_host
        a.to_host = lambda arr: (self.log.append(['to_host', self.where(arr.ctypes.data), int(arr.size)]), to_host(arr))[1]
        e.policy_f = self._stand_ins('policy', e)
        e.txlog_f = self._stand_ins('txlog', e)
        return ctx

    def _wrap(self, name, real):
        def call(*args):
            self.event(name, args)
            if name == 'group_create':
                rc = real(*args)
                self.members[args[2]._obj.value] = 'group'
                return rc
            return real(*args)
        return call

    def _alloc(self, kind, real):
        def alloc(n, dtype):
            arr = real(n, dtype)
            self.bufs.append(arr)
            self.log.append(['alloc', kind, int(n)])
            return arr
        return alloc

    def _stand_ins(self, what, engine):
        """engine.policy_f / engine.txlog_f as Python callables: *_run_days forwards to the engine's (or the group's) day
        entry point, policy_read_trace leaves the zeros it was given, everything else returns 0"""
        from reina_model_amd import policy as pol, txlog as txl
        owners = {}   # attachment handle -> handle of its engine or group
        raw = {n: engine.f[n] for n in ('run_days_hist', 'group_run_days')}

        def make(name):
            def call(*args):
                if name.endswith('_create'):
                    owner = args[0]
                    out = args[2]._obj
                    out.value = 0x1000 + len(owners)
                    owners[out.value] = owner
                    self.members[out.value] = '%s of %s' % (what, self.label(owner))
                self.event(name, args)
                if name == what + '_run_days':
                    return raw['run_days_hist'](owners[args[0].value], *args[1:])
                if name == 'group_%s_run_days' % what:
                    return raw['group_run_days'](owners[args[0].value], *args[1:])
                return 0
            return call
        return {n: make(n) for n in (pol.POLICY_FUNCTIONS if what == 'policy' else txl.TXLOG_FUNCTIONS)}


def _variables(scale=1.0, quiet=False):
    """the default scenario; scale: its mobility limits scaled (a sweep's members); quiet: without the interventions that
    change the contact tables, so that nothing cuts a chunk short"""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=12, icu_units=2)
    if quiet:
        v['interventions'] = [iv for iv in v['interventions'] if iv[0] not in ('limit-mobility', 'wear-masks')]
    if scale != 1.0:
        v['interventions'] = [[iv[0], iv[1], int(iv[2] * scale)] + list(iv[3:]) if iv[0] == 'limit-mobility' else list(iv)
                              for iv in v['interventions']]
    return v


class OneShardComm:
    """a communicator of one shard that asks for the collectives anyway (the phase-stepped route of Context.run); `log`: the
    recorder's, so the reductions of the read-back appear among the library calls"""
    rank, world, always_collective, attribution = 0, 1, True, 'mirror'

    def __init__(self, log):
        self.all_reduce_sum = lambda buf: log.append(['all_reduce_sum', int(np.asarray(buf).size)])
        self.all_reduce_max = lambda buf: log.append(['all_reduce_max', int(np.asarray(buf).size)])


def _ctx(rec, label, seed=SEEDS[0], policy=None, scale=1.0, log=False, quiet=False, comm=None):
    c = simulation.make_context(_variables(scale, quiet), age_counts=datasets.scaled_population(AGENTS), seed=seed, policy=policy,
                                engine_factory=par_backend.par_engine_factory, comm=comm)
    if rec is not None:
        rec.attach(c, label)
    if log:
        c.start_transmission_log()
    return c


def _digest(hist):
    return None if hist is None else [list(hist.shape), hashlib.sha256(np.ascontiguousarray(hist, dtype=np.int32).tobytes()).hexdigest()]


def _result(rec, hist, ctxs):
    out = dict(calls=rec.log[:], history=_digest(hist))
    out['mobility_history'] = [[float(x) for x in c.mobility_history] for c in ctxs]
    out['policy_levels'] = [None if c.policy_levels is None else [int(x) for x in c.policy_levels] for c in ctxs]
    out['day'] = [int(c.day) for c in ctxs]
    out['replayed'] = [bool(c._replayed) for c in ctxs]
    return out


def _plan(policy=None, scale=1.0):
    return _ctx(None, 'planner', scale=scale).make_plan(DAYS, policy=policy)


def scenario(name):
    """one way of running DAYS days of the default scenario, recorded: dict(calls, history, mobility_history, ...)"""
    rec = Recorder()
    pol = never_policy() if 'policy' in name else None
    log = 'txlog' in name
    hist_wanted = not name.endswith('_nohist')
    kind = name.replace('_nohist', '').replace('policy_', '').replace('txlog_', '').replace('quiet_', '').replace('sharded_', '')
    if kind == 'run':
        ctxs = [_ctx(rec, 'm0', policy=pol, log=log, quiet='quiet' in name, comm=OneShardComm(rec.log) if 'sharded' in name else None)]
        hist = ctxs[0].run(DAYS, record_history=hist_wanted)
    elif kind == 'plan':
        plan = _plan(pol)
        ctxs = [_ctx(rec, 'm0', policy=pol, log=log)]
        hist = ctxs[0].run_plan(plan, record_history=hist_wanted)
    elif kind == 'group':
        plan = _plan(pol)
        ctxs = [_ctx(rec, 'm%d' % m, seed=s) for m, s in enumerate(SEEDS)]
        hist = ensemble.run_group_plan(ctxs, plan, record_history=hist_wanted, policy=pol, txlog=log)
    elif kind == 'sweep':
        scales = (1.0, 0.5, 0.25)
        plans = [_plan(scale=s) for s in scales]
        ctxs = [_ctx(rec, 'm%d' % m, seed=s, scale=sc) for m, (s, sc) in enumerate(zip(SEEDS, scales))]
        hist = ensemble.run_group_plan(ctxs, plans[0], record_history=hist_wanted, member_plans=plans)
    else:
        raise KeyError(name)
    return _result(rec, hist, ctxs)


SCENARIOS = ('run', 'run_nohist', 'plan', 'plan_nohist', 'group', 'group_nohist', 'sweep',
             'policy_run', 'policy_run_nohist', 'policy_plan', 'policy_plan_nohist', 'policy_group', 'policy_group_nohist',
             'txlog_run', 'txlog_plan', 'txlog_group', 'quiet_run', 'policy_quiet_run', 'sharded_run', 'sharded_run_nohist')


@pytest.fixture(scope='module')
def expected():
    with open(TRACES) as f:
        return json.load(f)


@pytest.mark.parametrize('name', SCENARIOS)
def test_the_library_sees_the_calls_it_saw_before_the_day_runner(name, expected, monkeypatch):
    """the full call sequence (uploads, allocations and read-backs included), the history, the mobility history and the policy
    levels of every route equal the recorded ones"""
    monkeypatch.setattr(eng, 'is_device', lambda engine: True)   # (a Context keeps its log on the "device": the stand-ins)
    got = json.loads(json.dumps(scenario(name)))
    want = expected[name]
    assert len(got['calls']) == len(want['calls']), 'number of calls'
    for k, (g, w) in enumerate(zip(got['calls'], want['calls'])):
        assert g == w, 'call %d' % k
    for key in ('history', 'mobility_history', 'policy_levels', 'day', 'replayed'):
        assert got[key] == want[key], key


def test_the_scenario_crosses_table_changes_and_the_chunks_grow_to_64(expected):
    """what the recorded traces must contain to be worth comparing with: table uploads inside the run, chunks of 1, 2, 4 ... 64
    days, a forced flush before an upload, per-member uploads in the sweep, the policy's bank on the first day"""
    chunks = lambda name, entry: [e[2] for e in expected[name]['calls'] if e[0] == entry]
    assert chunks('quiet_run', 'run_days_hist') == [1, 2, 4, 8, 16, 32, 64, 64, 9]       # capped at 64
    assert chunks('policy_quiet_run', 'policy_run_days') == [1, 2, 4, 8, 16, 32, 64, 64, 9]
    run = expected['run']['calls']
    ns = chunks('run', 'run_days_hist')
    assert sum(ns) == DAYS and ns[:4] == [1, 2, 4, 8]
    ups = [k for k, e in enumerate(run) if e[0] == 'upload_contact_tables']
    assert len(ups) >= 2 and all(run[k - 1][0] == 'run_days_hist' for k in ups)          # pending days go first
    assert any(n not in (1, 2, 4, 8, 16, 32, 64) for n in ns[:-1])                        # (an upload cut a chunk short)
    sweep = expected['sweep']['calls']
    assert {e[1] for e in sweep if e[0] == 'upload_contact_tables'} == {'m0', 'm1', 'm2'}
    sharded = expected['sharded_run']['calls']
    assert sharded[0] == ['alloc', 'zeros', DAYS * eng.COUNTER_WORDS]                     # (a sharded history is zeroed)
    assert [e[0] for e in sharded].count('step_phase') == DAYS * eng.PH_NR and 'run_days_hist' not in [e[0] for e in sharded]
    assert [e[0] for e in sharded[-6:]] == ['to_host', 'all_reduce_sum', 'all_reduce_max', 'read_counters', 'all_reduce_sum', 'all_reduce_max']
    pol = expected['policy_run']['calls']
    first_day = next(k for k, e in enumerate(pol) if e[0] == 'policy_run_days')
    assert [e[0] for e in pol[:first_day]].count('policy_upload_level') == 2
    assert expected['policy_run_nohist']['calls'][-1][0] == 'read_counters'      # the policy routes wait ...
    assert expected['run_nohist']['calls'][-1][0] == 'run_days_hist'             # ... the plain ones do not


if __name__ == '__main__':
    if '--record' in sys.argv:
        eng.is_device = lambda engine: True
        with open(TRACES, 'w') as f:
            json.dump({name: scenario(name) for name in SCENARIOS}, f, separators=(',', ':'))
            f.write('\n')
