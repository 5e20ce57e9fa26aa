"""Snapshots on the MI355X (include/reina_snapshot.h: k_snap_count / k_snap_scan / k_snap_pack / k_snap_unpack): a restored
GPU run is the uninterrupted one, the GPU packer writes the numpy packer's bytes, a snapshot continues with a NEW seed on the
GPU exactly as on oracle B (both ways), an engine-group fork equals single restores, and a 5e7-agent state round-trips."""
import copy

import numpy as np
import pytest

import par_backend
from golden_util import load_run, variables_for
from reina_model_amd import datasets, ensemble, simulation, snapshot as snapmod
from reina_model_amd import engine as eng
from reina_model_amd.variables import VARIABLE_DEFAULTS

pytestmark = pytest.mark.gpu


def _host(ctx, name):
    return np.ascontiguousarray(ctx.engine.alloc.to_host(ctx.engine.tensors[name])).view(np.uint32)


def _bit_planes_ok(ctx):
    hot = _host(ctx, 'hot')
    n = len(hot)
    for name, want in (('active_bits', (hot & 0x8000) != 0), ('infected_bits', (hot & 7) != 0)):
        bits = np.unpackbits(_host(ctx, name).view(np.uint8), bitorder='little').astype(bool)
        assert np.array_equal(bits[:n], want), name
        assert not bits[n:].any(), name


def _same_state(a, b):
    from shard_util import list_pairs
    for c in (a, b):
        if isinstance(c.engine.alloc, eng.TorchAllocator):
            _bit_planes_ok(c)
    for name in ('hot', 'infector', 'n_infected', 'onset_days', 'vacc_day', 'counters'):
        assert np.array_equal(_host(a, name), _host(b, name)), name
    ca, cb = _host(a, 'control'), _host(b, 'control')
    for l, q in ((2, 'queue0'), (3, 'queue1')):
        assert ca[l] == cb[l], q
        assert np.array_equal(np.sort(_host(a, q)[:ca[l]]), np.sort(_host(b, q)[:cb[l]])), q
    assert np.array_equal(list_pairs(a), list_pairs(b)), 'infectee lists'


def _kitchen():
    _, meta = load_run('mini_kitchen_s0')
    return variables_for(meta), np.asarray(meta['age_counts']), meta['seed'], meta['interventions']


def _gpu(v, ages, seed, ivs=None, snap=None):
    return simulation.make_context(v, age_counts=ages, seed=seed, interventions=ivs, snapshot=snap)


def _cpu(v, ages, seed, ivs=None, snap=None):
    return simulation.make_context(v, age_counts=ages, seed=seed, interventions=ivs, snapshot=snap,
                                   engine_factory=par_backend.par_engine_factory)


def _hus():
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    return v, datasets.get_population_for_area('HUS')


def test_gpu_restore_equals_uninterrupted_gpu_run():
    """HUS x 150 days; snapshots before the first imports have spread (day 20), in the lock-down (day 70) and on a
    contact-tracing day with a test queue (day 125); bit planes rebuilt"""
    v, ages = _hus()
    a = _gpu(v, ages, 11)
    hist, snaps, done = [], {}, 0
    for d in (20, 70, 125):
        hist.append(a.run(d - done))
        done = d
        snaps[d] = a.snapshot()
    hist.append(a.run(150 - done))
    hist = np.concatenate(hist)
    assert snaps[125].header['testing_ever'] and sum(snaps[125].header['qlen']) > 0
    assert snaps[125].on_device and snaps[125].nbytes < 68 * a.total_people
    for d, s in snaps.items():
        b = _gpu(v, ages, 11, snap=s)
        assert np.array_equal(b.run(150 - d), hist[d:]), d
        _same_state(a, b)
        del b


def test_gpu_packer_writes_the_numpy_packers_bytes():
    v, ages, seed, ivs = _kitchen()
    g, c = _gpu(v, ages, seed, ivs), _cpu(v, ages, seed, ivs)
    assert np.array_equal(g.run(80), c.run(80))
    sg, sc = g.snapshot().to_host(), c.snapshot()
    wg, wc = sg.image.view(np.uint32), sc.image.view(np.uint32)
    assert sg.header['n_base'] == sc.header['n_base'] and sg.header['n_slot'] == sc.header['n_slot']
    assert sg.header['n_slot'] > 0 and sg.header['testing_ever'] == sc.header['testing_ever']
    lay = snapmod.layout(g.total_people, sg.header['n_base'], sg.header['n_slot'], sg.header['qlen'])
    assert np.array_equal(wg[lay['tb']:lay['q']], wc[lay['tb']:lay['q']]), 'tile tables and record streams'
    assert np.array_equal(wg[:snapmod.HEADER_WORDS], wc[:snapmod.HEADER_WORDS]), 'header'
    assert np.array_equal(wg[snapmod.HEADER_WORDS:snapmod.HEADER_WORDS + eng.COUNTER_WORDS],
                          wc[snapmod.HEADER_WORDS:snapmod.HEADER_WORDS + eng.COUNTER_WORDS]), 'counters'


def test_cross_engine_continuation_with_a_new_seed(tmp_path):
    v, ages, seed, ivs = _kitchen()
    new_seed = 4242
    # a GPU snapshot through a file into oracle B and into the GPU
    g = _gpu(v, ages, seed, ivs)
    g.run(70)
    path = str(tmp_path / 'g.rsnp')
    g.snapshot().save(path)
    b = _cpu(v, ages, new_seed, ivs, snap=snapmod.Snapshot.load(path))
    g2 = _gpu(v, ages, new_seed, ivs, snap=snapmod.Snapshot.load(path, device='cuda:0'))
    assert np.array_equal(g2.run(60), b.run(60))
    _same_state(g2, b)
    # an oracle-B snapshot restored on the GPU
    c = _cpu(v, ages, seed, ivs)
    c.run(70)
    sc = c.snapshot()
    g3, b3 = _gpu(v, ages, new_seed, ivs, snap=sc), _cpu(v, ages, new_seed, ivs, snap=sc)
    h3 = g3.run(60)
    assert np.array_equal(h3, b3.run(60))
    _same_state(g3, b3)
    assert not np.array_equal(h3, c.run(60))   # (the new seed changes the future)


def test_group_fork_equals_single_restores():
    v, ages = _hus()
    a = _gpu(v, ages, 5)
    a.run(100)
    snap = a.snapshot()
    seeds = [5] + [100 + k for k in range(15)]
    hist, members = ensemble.run_branches(snap, v, seeds, 30, age_counts=ages)
    assert hist.shape == (16, 30, eng.COUNTER_WORDS)
    assert np.array_equal(hist[0], a.run(30))
    for m, sd in enumerate(seeds):
        one = _gpu(v, ages, sd, snap=snap)
        assert np.array_equal(one.run(30), hist[m]), m
        _same_state(one, members[m])
        del one
    host = snap.to_host()
    for m in (1, 9):
        b = _cpu(v, ages, seeds[m], snap=host)
        assert np.array_equal(b.run(30), hist[m]), m
        _same_state(members[m], b)
    assert not np.array_equal(hist[1], hist[2])


def test_scale_5e7_agents_pack_unpack_continue():
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ages = datasets.scaled_population(50_000_000)
    a = _gpu(v, ages, 2)
    a.run(120, record_history=False)
    snap = a.snapshot()
    dense = 4 * a.total_people * (1 + eng.COLD_WORDS + eng.INLINE_INFECTEES)
    assert snap.nbytes < dense
    b = _gpu(v, ages, 2, snap=snap)
    del snap
    ha, hb = a.run(10), b.run(10)
    assert np.array_equal(ha, hb)
    assert np.array_equal(a.engine.read_counters(), b.engine.read_counters())
    assert np.array_equal(_host(a, 'hot'), _host(b, 'hot'))
