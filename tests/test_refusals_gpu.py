"""What the library answers when it refuses: the return code and the text of reina_last_error(), word for word, of every
refusal of the C ABI that arguments alone can reach -- on one engine of 1027 agents (two tiles and three agents, N mod 4 = 3)
and on a group of three such engines, with a log and a course attached to each.  Every case is refused on the host, before
anything is queued: no kernel runs on a bad argument, and after each refused call the counters and the log words of member 0
are what they were.

The expected answers (tests/test_refusals_gpu.json) were recorded with this very file on commit 916234f, the last one on which
every site of the host code assigned the text and returned the code by hand: `python tests/test_refusals_gpu.py --record`
rewrites the file from the library as it stands, which is only ever right on a commit whose answers are the ones to keep.
(The texts HIP_CHECK builds from a spelled-out expression are no part of this: they move with the code.)

A bare code comes with the text of the refusal before it, so the cases run in one fixed order, all of them, whichever are asked for."""
import ctypes
import functools
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]   # (for `python tests/test_refusals_gpu.py --record`)
import policy_util as pu
import snap_util
import summary_util as su
from reina_model_amd import course as crs
from reina_model_amd import engine as eng
from reina_model_amd import lineage as lin, policy as pol, summary as sm, transmission as tx, txlog as txl

pytestmark = pytest.mark.gpu

RECORDED = os.path.join(HERE, 'test_refusals_gpu.json')
N_AGENTS, MEMBERS = 1027, 3
N_DAYS, PERIOD, PERIODS = 8, 7, 4           # of the calls that are taken
UNTOUCHED = -77                             # what the report buffer holds while nothing writes it


def _collect():
    """{case: [return code, last_error text]} in the order the cases ran"""
    import torch
    ctx = snap_util.make_context(N_AGENTS)
    members = [snap_util.make_context(N_AGENTS) for _ in range(MEMBERS)]
    e, engines = ctx.engine, [c.engine for c in members]
    group = eng.EngineGroup(engines)
    log, glog = txl.DeviceLog(e), txl.DeviceLog(engines[0], group=group)
    course, gcourse = crs.DeviceCourse(log), crs.DeviceCourse(glog)
    rule = pol.Policy(pol.Signal('in_ward', 'increment', 7), pu.ladder(2), up=[5], down=[1])
    policy, gpolicy = pol.DevicePolicy(rule, pu.START_DATE, engine=e), pol.DevicePolicy(rule, pu.START_DATE, group=group)
    f, stream, dev = e.f, e.alloc.stream(), e.alloc.device
    out = {}

    def state():
        torch.cuda.synchronize()
        words = []
        for x in (e, engines[0]):
            c = np.zeros(eng.COUNTER_WORDS, dtype=np.int32)
            assert f['read_counters'](x._h, c.ctypes.data, stream) == 0
            words.append(c)
        return words + [log.words(0), glog.words(0), course.words(0), gcourse.words(0)]

    def refused(name, rc):
        assert name not in out, name
        out[name] = [int(rc), (f['last_error']() or b'').decode()]
        assert rc != 0, name
        for a, b in zip(state(), before):
            assert np.array_equal(a, b), '%s queued something' % name

    # ------------------------------------------------------------------------------------------ the reports
    scratch_bytes = max(lin.scratch_bytes(N_AGENTS), tx.scratch_bytes(N_AGENTS)) + 16
    scratch = [torch.empty(scratch_bytes, dtype=torch.uint8, device=dev) for _ in range(MEMBERS)]
    words = max(tx.REPORT_WORDS, txl.report_words(N_DAYS), crs.report_words(N_DAYS), lin.report_words(PERIODS))
    rep = torch.zeros(MEMBERS * words + 2, dtype=torch.int64, device=dev)
    table = np.zeros(eng.MAX_AGES, dtype=np.uint8)
    high = table.copy()
    high[5] = 3                                                     # (with n_groups = 3: not below it)
    good = dict(table=table.ctypes.data, ng=3, n_days=N_DAYS, pd=PERIOD, P=PERIODS, rep=rep.data_ptr(), s_off=0, m_off=0)

    def pointers(a):
        return (ctypes.c_void_p * MEMBERS)(*[scratch[m].data_ptr() + (a['m_off'] if m == 1 else 0) for m in range(MEMBERS)])

    reports = {   # name -> (max groups, kinds of argument beside the table and the report, the call)
        'tx_report': (tx.MAX_GROUPS, 'scratch', lambda a: e.tx_f['tx_report'](
            e._h, a['table'], a['ng'], 0, scratch[0].data_ptr() + a['s_off'], a['rep'], stream)),
        'group_tx_report': (tx.MAX_GROUPS, 'member_scratch', lambda a: e.tx_f['group_tx_report'](
            group._h, a['table'], a['ng'], 0, pointers(a), a['rep'], stream)),
        'txlog_report': (txl.MAX_GROUPS, 'n_days', lambda a: e.txlog_f['txlog_report'](
            log._h, a['table'], a['ng'], a['n_days'], a['rep'], stream)),
        'group_txlog_report': (txl.MAX_GROUPS, 'n_days', lambda a: e.txlog_f['group_txlog_report'](
            glog._h, a['table'], a['ng'], a['n_days'], a['rep'], stream)),
        'course_report': (crs.MAX_GROUPS, 'n_days', lambda a: e.course_f['course_report'](
            course._h, a['table'], a['ng'], a['n_days'], a['rep'], stream)),
        'course_report_of_a_group': (crs.MAX_GROUPS, 'n_days', lambda a: e.course_f['course_report'](
            gcourse._h, a['table'], a['ng'], a['n_days'], a['rep'], stream)),
        'lineage_report': (lin.MAX_GROUPS, 'scratch periods', lambda a: e.lineage_f['lineage_report'](
            log._h, a['table'], a['ng'], a['pd'], a['P'], 0, scratch[0].data_ptr() + a['s_off'], a['rep'], stream)),
        'group_lineage_report': (lin.MAX_GROUPS, 'member_scratch periods', lambda a: e.lineage_f['group_lineage_report'](
            glog._h, a['table'], a['ng'], a['pd'], a['P'], 0, pointers(a), a['rep'], stream)),
    }
    for name, (_, _, call) in reports.items():                      # the arguments every refusal below departs from are taken
        assert call(good) == 0, (name, f['last_error']())
    torch.cuda.synchronize()
    rep.fill_(UNTOUCHED)
    before = state()
    for name, (max_groups, kinds, call) in reports.items():
        cases = [('table_null', dict(table=None)), ('n_groups_0', dict(ng=0)), ('n_groups_over', dict(ng=max_groups + 1)),
                 ('group_not_below_n_groups', dict(table=high.ctypes.data)),
                 ('report_null', dict(rep=None)), ('report_misaligned', dict(rep=rep.data_ptr() + 4))]
        if 'n_days' in kinds:
            cases += [('n_days_0', dict(n_days=0)), ('n_days_over', dict(n_days=eng.MAX_DAYS + 1))]
        if 'member_scratch' in kinds:
            cases += [('member_scratch_misaligned', dict(m_off=4))]
        elif 'scratch' in kinds:
            cases += [('scratch_misaligned', dict(s_off=4))]
        if 'periods' in kinds:
            cases += [('period_days_0', dict(pd=0)), ('period_days_over', dict(pd=eng.MAX_DAYS + 1)),
                      ('n_periods_0', dict(P=0)), ('n_periods_over', dict(P=lin.MAX_PERIODS + 1))]
        for case, kw in cases:
            refused('%s-%s' % (name, case), call(dict(good, **kw)))
    # two arguments wrong: the one that was reported before
    refused('txlog_report-n_groups_0_and_n_days_0', reports['txlog_report'][2](dict(good, ng=0, n_days=0)))
    refused('txlog_report-n_days_0_and_report_null', reports['txlog_report'][2](dict(good, n_days=0, rep=None)))
    refused('lineage_report-period_days_0_and_scratch_misaligned', reports['lineage_report'][2](dict(good, pd=0, s_off=4)))
    refused('group_lineage_report-n_periods_0_and_member_scratch_misaligned',
            reports['group_lineage_report'][2](dict(good, P=0, m_off=4)))
    refused('group_tx_report-n_groups_0_and_member_scratch_misaligned', reports['group_tx_report'][2](dict(good, ng=0, m_off=4)))
    refused('group_tx_report-scratch_null', e.tx_f['group_tx_report'](group._h, good['table'], 3, 0, None, good['rep'], stream))
    refused('group_lineage_report-scratch_null',
            e.lineage_f['group_lineage_report'](glog._h, good['table'], 3, PERIOD, PERIODS, 0, None, good['rep'], stream))

    # ------------------------------------------------------------------------------------------ one engine's for a group's
    days = (eng.Day * 1)()
    one, ptrs = scratch[0].data_ptr(), pointers(good)
    for name, rc in (
            ('txlog_run_days-of_a_group', lambda: e.txlog_f['txlog_run_days'](glog._h, days, 1, None, stream)),
            ('group_txlog_run_days-of_one_engine', lambda: e.txlog_f['group_txlog_run_days'](log._h, days, 1, None, stream)),
            ('txlog_report-of_a_group', lambda: e.txlog_f['txlog_report'](glog._h, good['table'], 3, N_DAYS, good['rep'], stream)),
            ('group_txlog_report-of_one_engine', lambda: e.txlog_f['group_txlog_report'](log._h, good['table'], 3, N_DAYS, good['rep'], stream)),
            ('lineage_report-of_a_group', lambda: e.lineage_f['lineage_report'](glog._h, good['table'], 3, PERIOD, PERIODS, 0, one, good['rep'], stream)),
            ('group_lineage_report-of_one_engine', lambda: e.lineage_f['group_lineage_report'](log._h, good['table'], 3, PERIOD, PERIODS, 0, ptrs, good['rep'], stream)),
            ('policy_run_days-of_a_group', lambda: e.policy_f['policy_run_days'](gpolicy._h, days, 1, None, stream)),
            ('group_policy_run_days-of_one_engine', lambda: e.policy_f['group_policy_run_days'](policy._h, days, 1, None, stream)),
            ('txlog_run_days-days_null', lambda: e.txlog_f['txlog_run_days'](log._h, None, 1, None, stream)),
            ('txlog_run_days-log_null', lambda: e.txlog_f['txlog_run_days'](None, days, 1, None, stream))):
        refused(name, rc())

    # ------------------------------------------------------------------------------------------ the logs
    host = np.zeros(N_AGENTS, dtype=np.uint64)
    for name, fn, h, member in (('txlog_read', e.txlog_f['txlog_read'], log._h, 1), ('txlog_write', e.txlog_f['txlog_write'], log._h, 1),
                                ('txlog_read-of_a_group', e.txlog_f['txlog_read'], glog._h, MEMBERS),
                                ('txlog_write-of_a_group', e.txlog_f['txlog_write'], glog._h, MEMBERS),
                                ('course_read', e.course_f['course_read'], course._h, 1), ('course_write', e.course_f['course_write'], course._h, 1),
                                ('course_read-of_a_group', e.course_f['course_read'], gcourse._h, MEMBERS),
                                ('course_write-of_a_group', e.course_f['course_write'], gcourse._h, 2 ** 32 - 1)):
        refused(name + '-member_out_of_range', fn(h, member, host.ctypes.data, stream))
        refused(name + '-host_null', fn(h, 0, None, stream))
    refused('txlog_record_day-max_days', e.txlog_f['txlog_record_day'](log._h, eng.MAX_DAYS, stream))
    refused('txlog_record_day-max_days-of_a_group', e.txlog_f['txlog_record_day'](glog._h, eng.MAX_DAYS, stream))
    days[0].day = eng.MAX_DAYS
    refused('txlog_run_days-max_days', e.txlog_f['txlog_run_days'](log._h, days, 1, None, stream))
    refused('group_txlog_run_days-max_days', e.txlog_f['group_txlog_run_days'](glog._h, days, 1, None, stream))
    h = ctypes.c_void_p()
    refused('course_create-log_has_one', e.course_f['course_create'](log._h, stream, ctypes.byref(h)))
    refused('course_create-group_log_has_one', e.course_f['course_create'](glog._h, stream, ctypes.byref(h)))
    assert not h.value
    log2 = txl.DeviceLog(e)
    course2 = crs.DeviceCourse(log2)
    assert e.txlog_f['txlog_destroy'](log2._h) == 0                 # (the log goes first: the course refuses from then on)
    log2._h, log2.course = ctypes.c_void_p(), None
    refused('course_report-log_gone', e.course_f['course_report'](course2._h, good['table'], 3, N_DAYS, good['rep'], stream))
    refused('course_read-log_gone', e.course_f['course_read'](course2._h, 0, host.ctypes.data, stream))
    refused('course_write-log_gone', e.course_f['course_write'](course2._h, 0, host.ctypes.data, stream))
    course2.close()

    # ------------------------------------------------------------------------------------------ the clones
    def pairs(p):
        flat = [x for pr in p for x in pr]
        return (ctypes.c_uint32 * max(len(flat), 1))(*flat), len(p)

    lists = (('destination_twice', [(1, 0), (1, 2)]), ('source_is_destination', [(1, 0), (0, 2)]), ('onto_itself', [(2, 2)]),
             ('destination_out_of_range', [(MEMBERS, 0)]), ('source_out_of_range', [(1, 0), (2, 70000)]))
    for name, fn, h in (('group_clone', e.filter_f['group_clone'], group._h), ('group_txlog_clone', e.filter_log_f['group_txlog_clone'], glog._h)):
        refused(name + '-no_pair_list', fn(h, None, 1, stream))
        for case, p in lists:
            refused('%s-%s' % (name, case), fn(h, *pairs(p), stream))
    refused('group_clone-group_null', e.filter_f['group_clone'](None, *pairs([(1, 0)]), stream))
    refused('group_txlog_clone-no_log', e.filter_log_f['group_txlog_clone'](None, *pairs([(1, 0)]), stream))
    refused('group_txlog_clone-of_one_engine', e.filter_log_f['group_txlog_clone'](log._h, *pairs([(0, 0)]), stream))

    # ------------------------------------------------------------------------------------------ the policy
    for name, create, owner in (('policy_create', e.policy_f['policy_create'], e._h), ('group_policy_create', e.policy_f['group_policy_create'], group._h)):
        for field, value in (('n_levels', 1), ('n_levels', pol.MAX_LEVELS + 1), ('signal', 2 ** 31), ('kind', 7), ('n_days', 0), ('n_days', 29),
                             ('review_every', 0), ('start_day', eng.MAX_DAYS), ('start_day', 2 ** 32 - 1), ('up', None), ('down', None)):
            r = pol.Policy(pol.Signal('in_ward', 'increment', 7), pu.ladder(3), up=[5, 9], down=[1, 2]).rule_abi(pu.START_DATE)
            if field == 'up':
                r.up[1] = 4                                         # (decreasing)
            elif field == 'down':
                r.down[0] = 6                                       # (above up[0])
            else:
                setattr(r, field, value)
            h = ctypes.c_void_p()
            refused('%s-%s_%s' % (name, field, value), create(owner, ctypes.byref(r), ctypes.byref(h)))
            assert not h.value
        refused(name + '-rule_null', create(owner, None, ctypes.byref(h)))
    zeros = [np.zeros(8 * eng.MAX_AGES, dtype=np.float32) for _ in range(5)]
    t, _keep = eng.Engine._tables_abi(*zeros, [(0, 100)])
    trace = np.zeros((MEMBERS, 2, pol.TRACE_WORDS), dtype=np.int32)
    days[0].day = 0
    late = (eng.Day * 2)()
    late[1].day = eng.MAX_DAYS
    for name, p, run in (('policy', policy, e.policy_f['policy_run_days']), ('group_policy', gpolicy, e.policy_f['group_policy_run_days'])):
        refused(name + '_upload_level-level_out_of_range', e.policy_f['policy_upload_level'](p._h, 2, ctypes.byref(t), stream))
        refused(name + '_upload_level-tables_null', e.policy_f['policy_upload_level'](p._h, 0, None, stream))
        refused(name + '_read_trace-range', e.policy_f['policy_read_trace'](p._h, eng.MAX_DAYS - 1, 2, trace.ctypes.data, stream))
        refused(name + '_read_trace-out_null', e.policy_f['policy_read_trace'](p._h, 0, 2, None, stream))
        refused(name + '_run_days-a_day_beyond_behind_a_good_one', run(p._h, late, 2, None, stream))
        refused(name + '_run_days-never_uploaded', run(p._h, days, 1, None, stream))
        refused(name + '_run_days-days_null', run(p._h, None, 1, None, stream))
    assert not trace.any()

    # ------------------------------------------------------------------------------------------ snapshots
    image = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    refused('snap_pack-null', e.snap_f['snap_pack'](e._h, None, 1 << 16, stream))
    refused('snap_pack-misaligned', e.snap_f['snap_pack'](e._h, image.data_ptr() + 4, 1 << 16, stream))
    refused('snap_pack-too_small', e.snap_f['snap_pack'](e._h, image.data_ptr(), 16, stream))
    refused('snap_unpack-null', e.snap_f['snap_unpack'](e._h, None, stream))
    refused('snap_unpack-misaligned', e.snap_f['snap_unpack'](e._h, image.data_ptr() + 4, stream))
    refused('snap_unpack-zeroed_header', e.snap_f['snap_unpack'](e._h, image.data_ptr(), stream))
    refused('group_snap_unpack-misaligned', e.snap_f['group_snap_unpack'](group._h, image.data_ptr() + 4, stream))
    refused('group_snap_unpack-zeroed_header', e.snap_f['group_snap_unpack'](group._h, image.data_ptr(), stream))
    assert not bool(image.any())
    size = ctypes.c_uint64()
    assert e.snap_f['snap_measure'](e._h, ctypes.byref(size), stream) == 0
    whole = torch.zeros(size.value // 4, dtype=torch.int32, device=dev)
    assert e.snap_f['snap_pack'](e._h, whole.data_ptr(), size.value, stream) == 0
    from reina_model_amd import snapshot as snp
    header = whole[:snp.HEADER_WORDS].cpu().numpy().view(np.uint32)
    assert header[snp.H_MAGIC] == snp.MAGIC and header[snp.H_N_AGENTS] == N_AGENTS
    for case, word, value in (('version', snp.H_VERSION, header[snp.H_VERSION] + 1), ('n_agents', snp.H_N_AGENTS, N_AGENTS + 1),
                              ('nr_ages', snp.H_NR_AGES, header[snp.H_NR_AGES] - 1), ('nr_variants', snp.H_NR_VARIANTS, header[snp.H_NR_VARIANTS] + 1),
                              ('n_base_over', snp.H_N_BASE, N_AGENTS + 1), ('n_slot_over_n_base', snp.H_N_SLOT, header[snp.H_N_BASE] + 1),
                              ('queue_over', snp.H_LEN_Q1, e.config.max_queue + 1), ('ages_hash', snp.H_AGES_HASH, header[snp.H_AGES_HASH] ^ 1),
                              ('disease_hash', snp.H_DISEASE_HASH + 1, header[snp.H_DISEASE_HASH + 1] ^ 1),
                              ('n_tiles', snp.H_N_TILES, header[snp.H_N_TILES] + 1), ('bytes', snp.H_BYTES, header[snp.H_BYTES] + 4)):
        bad = whole.clone()                                         # (a whole image: only its header is wrong)
        bad[word] = int(np.array(value, dtype=np.uint32).view(np.int32))
        refused('snap_unpack-header_' + case, e.snap_f['snap_unpack'](e._h, bad.data_ptr(), stream))
        refused('group_snap_unpack-header_' + case, e.snap_f['group_snap_unpack'](group._h, bad.data_ptr(), stream))

    # ------------------------------------------------------------------------------------------ contact tables, the engine
    A = e.config.nr_ages
    nrc, count = np.ones(eng.MAX_AGES, dtype=np.float32), np.ones(eng.MAX_AGES, dtype=np.int32)

    def tables(n_ranges=1, **at_40):
        c = count.copy()
        c[40] = at_40.get('count', 1)
        tab, keep = eng.Engine._tables_abi(nrc, c, zeros[2], zeros[3], zeros[4], [(0, A - 1)])
        tab.n_ranges = n_ranges
        return tab, keep

    for name, fn, owner in (('upload_contact_tables', f['upload_contact_tables'], e._h),
                            ('group_upload_contact_tables', f['group_upload_contact_tables'], group._h),
                            ('policy_upload_level', lambda h, tab, s: e.policy_f['policy_upload_level'](h, 0, tab, s), policy._h)):
        for case, kw in (('count_below_0', dict(count=-1)), ('count_over', dict(count=eng.MAX_ENTRIES + 1)),
                         ('ranges_over', dict(n_ranges=eng.MAX_RANGES + 1)), ('contacts_but_no_entries', dict(count=0))):
            tab, _keep = tables(**kw)
            refused('%s-%s' % (name, case), fn(owner, ctypes.byref(tab), stream))
    cfg = lambda **kw: _config(e.config, **kw)
    disease, h = eng.Disease(), ctypes.c_void_p()
    for case, c in (('nr_ages_0', cfg(nr_ages=0)), ('nr_ages_over', cfg(nr_ages=eng.MAX_AGES + 1)), ('nr_variants_0', cfg(nr_variants=0)),
                    ('age_start_decreasing', cfg(age_start_5=N_AGENTS + 1)), ('n_shards_over', cfg(n_shards=1000)),
                    ('shard_rank_over', cfg(n_shards=2, shard_rank=2)), ('mirror_slots_3', cfg(mirror_slots=3)),
                    ('exact_without_tables', cfg(n_shards=2, exact_attribution=1)), ('hosp_ranges_17', cfg(hosp_ranges=17)),
                    ('hosp_ranges_8', cfg(hosp_ranges=8)), ('max_hosp_events_over', cfg(n_shards=2, max_hosp_events=2 ** 30))):
        refused('create-' + case, f['create'](ctypes.byref(c), ctypes.byref(disease), ctypes.byref(h)))
        assert not h.value
    refused('create-config_null', f['create'](None, ctypes.byref(disease), ctypes.byref(h)))
    refused('bind_buffers-null_pointer', f['bind_buffers'](e._h, ctypes.byref(eng.Buffers())))
    day = eng.Day()
    day.day = eng.MAX_DAYS
    refused('step_day-max_days', f['step_day'](e._h, ctypes.byref(day), stream))
    day.day, day.n_import_batches = 0, 1000
    refused('step_day-import_batches_over', f['step_day'](e._h, ctypes.byref(day), stream))
    refused('step_phase-phase_out_of_range', f['step_phase'](e._h, ctypes.byref(eng.Day()), 99, stream))
    other = snap_util.make_context(700)
    hs = (ctypes.c_void_p * 2)(e._h, other.engine._h)
    refused('group_create-another_population', f['group_create'](hs, 2, ctypes.byref(h)))
    assert not h.value

    # ------------------------------------------------------------------------------------------ the summary
    _summary(refused)
    torch.cuda.synchronize()
    assert bool((rep == UNTOUCHED).all()), 'a refused call queued something'
    for x in (policy, gpolicy, course, gcourse, log, glog, group):
        x.close()
    return out


def _config(base, **kw):
    c = eng.Config.from_buffer_copy(base)
    c.shard_age_start = None
    for k, v in kw.items():
        if k.startswith('age_start_'):
            c.age_start[int(k[10:])] = v
        else:
            setattr(c, k, v)
    return c


def _summary(refused):
    """every refusal tests/test_summary_gpu.py lists, on its shapes"""
    import torch
    f = sm.library()
    K, days, nr_ages, G = 3, 2, 10, 2
    S = sm.n_series(G)
    h = torch.from_numpy(su.history(K, days, nr_ages, 'random')).to('cuda:0')
    row = 4 * eng.COUNTER_WORDS
    scratch = torch.empty(sm.scratch_bytes(K, days, S) + 16, dtype=torch.uint8, device='cuda:0')
    rep = torch.full((sm.report_words(K, days, S, 2, 1) + 2,), UNTOUCHED, dtype=torch.int64, device='cuda:0')
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(bases=[h.data_ptr() + m * days * row for m in range(K)], K=K, days=days, nr_ages=nr_ages,
                table=np.arange(eng.MAX_AGES, dtype=np.uint8) % G, G=G, ranks=np.array([0, 2], dtype=np.uint32), Q=2,
                thr=[(5, 1)], T=1, scratch=scratch.data_ptr(), rep=rep.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        bases = (ctypes.c_void_p * max(len(a['bases']), 1))(*a['bases']) if a['bases'] is not None else None
        thr = (sm.Threshold * max(len(a['thr']), 1))(*[sm.Threshold(s, v) for s, v in a['thr']]) if a['thr'] is not None else None
        table = np.ascontiguousarray(a['table'], dtype=np.uint8) if a['table'] is not None else None
        ranks = np.ascontiguousarray(a['ranks'], dtype=np.uint32) if a['ranks'] is not None else None
        return f['summary'](bases, a['K'], a['days'], a['nr_ages'], table.ctypes.data if table is not None else None, a['G'],
                            ranks.ctypes.data if ranks is not None else None, a['Q'], thr, a['T'], a['scratch'], a['rep'], stream)

    bad_table = good['table'].copy()
    bad_table[nr_ages - 1] = G
    for name, kw in (
            ('K_0', dict(K=0)), ('K_over', dict(K=1025, bases=good['bases'] * 342)), ('days_0', dict(days=0)), ('days_over', dict(days=eng.MAX_DAYS + 1)),
            ('nr_ages_0', dict(nr_ages=0)), ('nr_ages_over', dict(nr_ages=eng.MAX_AGES + 1)), ('n_groups_0', dict(G=0)), ('n_groups_over', dict(G=17)),
            ('n_ranks_over', dict(Q=17)), ('n_thresholds_over', dict(T=33)), ('group_not_below_n_groups', dict(table=bad_table)),
            ('rank_not_below_K', dict(ranks=np.array([0, K], dtype=np.uint32))), ('series_not_below_S', dict(thr=[(S, 0)])),
            ('bases_null', dict(bases=None)), ('table_null', dict(table=None)), ('ranks_null', dict(ranks=None)), ('thresholds_null', dict(thr=None)),
            ('scratch_null', dict(scratch=None)), ('report_null', dict(rep=None)),
            ('a_member_null', dict(bases=[good['bases'][0], 0, good['bases'][2]])),
            ('a_member_misaligned', dict(bases=[good['bases'][0], good['bases'][1] + 4, good['bases'][2]])),
            ('scratch_misaligned', dict(scratch=good['scratch'] + 4)), ('report_misaligned', dict(rep=good['rep'] + 4))):
        refused('summary-' + name, call(**kw))
    torch.cuda.synchronize()
    assert bool((rep == UNTOUCHED).all()), 'a refused reina_summary queued something'


@functools.lru_cache(maxsize=None)
def _got():
    return _collect()


def _recorded():
    with open(RECORDED) as f:
        return json.load(f)


@pytest.mark.parametrize('name', sorted(_recorded()) if os.path.exists(RECORDED) else [])
def test_every_refusal_has_the_code_and_the_text_it_had(name):
    assert _got()[name] == _recorded()[name]


def test_the_recorded_cases_are_the_cases_of_this_file_and_say_why():
    """all names of this file and no others; every code negative; a text with every refusal that names its reason (the bare
    codes -- a null handle or list -- come with the text of the refusal before them)"""
    want, got = _recorded(), _got()
    assert sorted(want) == sorted(got)
    assert len(want) >= 200
    assert all(rc < 0 for rc, _ in want.values())
    for name, words in (('txlog_report-n_days_0', 'txlog report: n_days'), ('course_report-report_misaligned', '16-byte aligned'),
                        ('group_lineage_report-member_scratch_misaligned', "every member's scratch"),
                        ('group_txlog_clone-source_is_destination', 'reina_group_txlog_clone: a source is also a destination'),
                        ('summary-K_0', 'reina_summary: K must be'), ('snap_unpack-zeroed_header', 'magic'),
                        ('upload_contact_tables-contacts_but_no_entries', 'age 40 has contacts')):
        assert words in want[name][1], name


if __name__ == '__main__':
    if '--record' in sys.argv:
        with open(RECORDED, 'w') as f:
            json.dump(_collect(), f, indent=0, sort_keys=True)
            f.write('\n')
