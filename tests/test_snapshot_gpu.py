"""Snapshots on the MI355X (include/reina_snapshot.h: k_snap_count / k_snap_scan / k_snap_pack / k_snap_unpack): a restored
GPU run is the uninterrupted one, the GPU packer writes the numpy packer's bytes, a snapshot continues with a NEW seed on the
GPU exactly as on oracle B (both ways), ragged populations snapshot as on oracle B, an engine-group fork (large and small
populations) equals single restores, and a 5e7-agent state packs to the format and round-trips."""
import copy

import numpy as np
import pytest

import par_backend
import snap_util
from golden_util import load_run, variables_for
from reina_model_amd import datasets, ensemble, simulation, snapshot as snapmod
from reina_model_amd import engine as eng
from reina_model_amd.model import NO_TESTING
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


# words of the control block that carry state from one day to the next in both engines: the queue lengths and the
# vaccination cursors (include/reina_hip.h REINA_L_*).  The others are the day's list lengths, tickets and diagnostics, which
# each engine keeps its own way (the GPU's day-open word, active-agent counts and hospital peak; oracle B's list lengths)
# and resets before it reads them (test_cross_engine_continuation_with_a_new_seed).
CARRIED_CONTROL = [2, 3, 4] + list(range(32, 48))


def _assert_image_equals_oracle_bs(wg, wc):
    """a GPU image against oracle B's of the same state: every word but the control block's per-day words; the queues
    as multisets (the GPU appends to them with atomics, in no fixed order; _same_state compares them so too)"""
    assert len(wg) == len(wc)
    g, c = wg.view(np.uint32), wc.view(np.uint32)
    h = snapmod.parse_header(c)
    lay = snapmod.layout(h['n_agents'], h['n_base'], h['n_slot'], h['qlen'])
    at = snapmod.HEADER_WORDS + eng.COUNTER_WORDS
    same = np.ones(lay['q'], dtype=bool)
    same[at:at + eng.L_NR] = False
    same[at + np.array(CARRIED_CONTROL)] = True
    bad = np.flatnonzero((g[:lay['q']] != c[:lay['q']]) & same)
    assert len(bad) == 0, 'words %s differ: %s != %s' % (bad[:8], g[bad[:8]], c[bad[:8]])
    q = lay['q']
    for k, n in enumerate(h['qlen']):
        assert np.array_equal(np.sort(g[q:q + n]), np.sort(c[q:q + n])), 'queue %d' % k
        q += n
    assert q == len(c)


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
    assert sg.header['n_base'] == sc.header['n_base'] and sg.header['n_slot'] == sc.header['n_slot']
    assert sg.header['n_slot'] > 0 and sg.header['testing_ever'] == sc.header['testing_ever']
    # the whole image: header, counters, the carried control words, tile tables, pad, record streams, queues
    _assert_image_equals_oracle_bs(sg.image, sc.image)


@pytest.mark.parametrize('total', [4099, 10007])
def test_ragged_population_snapshot_is_oracle_bs_and_continues(total):
    """test_parity_gpu's ragged populations (N not a multiple of the tile, nor of the wave): on day 60 the GPU image is oracle
    B's byte for byte but for the control block's per-day words, and a GPU restore runs to day 120 as the uninterrupted run"""
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    v.update(hospital_beds=3, icu_units=1)
    ages = datasets.scaled_population(total)
    g, c = _gpu(v, ages, 11), _cpu(v, ages, 11)
    assert np.array_equal(g.run(60), c.run(60))
    sg, sc = g.snapshot(), c.snapshot()
    wg, wc = sg.to_host().image, sc.image
    assert sc.header['n_base'] > 0 and total % snapmod.TILE != 0
    _assert_image_equals_oracle_bs(wg, wc)
    b = _gpu(v, ages, 11, snap=sg)
    assert np.array_equal(b.run(60), g.run(60))
    _same_state(g, b)


def test_small_population_fork_equals_single_restores():
    """the kitchen-sink run forked on day 70 into 40 seeds (T = 59 tiles: the group unpack splits the members over several
    chunks of blockIdx.y, the last one ragged on a 256-CU chip); every member is the single restore with its seed"""
    import torch
    v, ages, seed, ivs = _kitchen()
    v = dict(v, simulation_days=200)
    a = _gpu(v, ages, seed, ivs)
    a.run(70)
    snap = a.snapshot()
    seeds = [seed] + [300 + k for k in range(39)]
    chunks, per, last = snap_util.group_geometry(snap.header['n_tiles'], len(seeds),
                                                 torch.cuda.get_device_properties(0).multi_processor_count)
    assert chunks > 1, (chunks, per, last)
    hist, members = ensemble.run_branches(snap, v, seeds, 30, age_counts=ages, interventions=ivs)
    assert hist.shape == (40, 30, eng.COUNTER_WORDS)
    assert np.array_equal(hist[0], a.run(30))
    for m, sd in enumerate(seeds):
        one = _gpu(v, ages, sd, ivs, snap=snap)
        assert np.array_equal(one.run(30), hist[m]), m
        _same_state(one, members[m])
        del one
    host = snap.to_host()
    for m in (1, 39):
        b = _cpu(v, ages, seeds[m], ivs, snap=host)
        assert np.array_equal(b.run(30), hist[m]), m
        _same_state(members[m], b)
    assert not np.array_equal(hist[1], hist[39])


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


class _HostCopy:
    """host copies of a HIP engine's persistent arrays, in the shape pack_numpy reads"""

    def __init__(self, ctx):
        self.config = ctx.engine.config
        self.tensors = {k: _host(ctx, k) for k in ('hot', 'cold', 'infectees', 'counters', 'control', 'queue0', 'queue1', 'level1')}


def test_scale_5e7_agents_pack_unpack_continue():
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    ages = datasets.scaled_population(50_000_000)
    a = _gpu(v, ages, 2)
    a.run(120, record_history=False)
    snap = a.snapshot()
    dense = 4 * a.total_people * (1 + eng.COLD_WORDS + eng.INLINE_INFECTEES)
    assert snap.nbytes < dense
    # the GPU image is the format of the engine's arrays (pack_numpy over host copies of them, 3.5 GB)
    want = snapmod.pack_numpy(_HostCopy(a), a._disease, a.testing_mode != NO_TESTING)
    got = snap.image.cpu().numpy()
    assert len(got) == len(want) and np.array_equal(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8]
    del want, got
    b = _gpu(v, ages, 2, snap=snap)
    del snap
    ha, hb = a.run(10), b.run(10)
    assert np.array_equal(ha, hb)
    assert np.array_equal(a.engine.read_counters(), b.engine.read_counters())
    assert np.array_equal(_host(a, 'hot'), _host(b, 'hot'))
    _same_state(a, b)
