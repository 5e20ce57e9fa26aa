"""The HIP == oracle B comparison, stated once: the pair of Contexts on the two engines, the per-agent state and bit planes
compared word for word, a run compared in chunks, the same on in-process shards.  `**context_kw` goes to simulation.make_context
on both sides (`disease=`: a ready disease block, parameters.expand_numpy; `strict=`: iterate() raises on the day of a problem).
tests/test_parity_gpu.py and tests/test_disease_blocks_gpu.py import these."""
import numpy as np

from reina_model_amd import engine as eng
from reina_model_amd import simulation


def _pair(variables, ages, seed, interventions=None, ipc=None, **context_kw):
    import par_backend
    gpu = simulation.make_context(variables, age_counts=ages, seed=seed, interventions=interventions, ipc=ipc, **context_kw)
    cpu = simulation.make_context(variables, age_counts=ages, seed=seed, interventions=interventions, ipc=ipc,
                                  engine_factory=par_backend.par_engine_factory, **context_kw)
    return gpu, cpu


def _assert_bit_planes(gpu):
    """the two per-agent bit planes of the HIP engine (include/reina_hip.h: active_bits, infected_bits) say what the hot
    words say: bit i of active_bits == the ACTIVE flag of hot[i] (what a sparse day's stream reads instead of the words),
    bit i of infected_bits == hot[i] is not SUSCEPTIBLE (what a contact looks its target up in); no bit beyond the agents"""
    t = gpu.engine.tensors
    hot = gpu.engine.alloc.to_host(t['hot']).view(np.uint32)
    n = len(hot)
    for name, want in (('active_bits', (hot & 0x8000) != 0), ('infected_bits', (hot & 7) != 0)):
        words = np.ascontiguousarray(gpu.engine.alloc.to_host(t[name]).view(np.uint32))
        bits = np.unpackbits(words.view(np.uint8), bitorder='little').astype(bool)
        assert np.array_equal(bits[:n], want), name
        assert not bits[n:].any(), name + ': bits beyond the last agent'


def _assert_state_equal(gpu, cpu):
    tg, tc = gpu.engine.tensors, cpu.engine.tensors
    if isinstance(gpu.engine.alloc, eng.TorchAllocator):   # (the HIP engine; the CPU checker keeps no bit planes)
        _assert_bit_planes(gpu)
    for name in ('hot', 'infector', 'n_infected', 'vacc_day'):
        a = gpu.engine.alloc.to_host(tg[name]).view(np.uint32)
        b = np.asarray(tc[name]).view(np.uint32)
        assert np.array_equal(a, b), name
    a = gpu.engine.alloc.to_host(tg['onset_days']).view(np.uint32)
    b = np.asarray(tc['onset_days']).view(np.uint32)
    assert np.array_equal(a, b), 'onset_days bits'
    cg = gpu.engine.alloc.to_host(tg['control'])
    cc = np.asarray(tc['control'])
    for l, q in ((2, 'queue0'), (3, 'queue1')):
        assert cg[l] == cc[l], 'queue length'
        qa = np.sort(gpu.engine.alloc.to_host(tg[q])[:cg[l]].view(np.uint32))
        qb = np.sort(np.asarray(tc[q])[:cc[l]].view(np.uint32))
        assert np.array_equal(qa, qb), q
    # infectee lists: same sets per infector (insertion order is free) -- EVERY inline slot and EVERY overflow chain (threaded
    # through the infectees' records, or through the pool's nodes under exact attribution: shard_util.list_pairs)
    from shard_util import list_pairs
    fa = gpu.engine.alloc.to_host(tg['first_infectee'])
    ia = gpu.engine.alloc.to_host(tg['infectees']).reshape(-1, eng.INLINE_INFECTEES)
    pa, pb = list_pairs(gpu), list_pairs(cpu)
    assert np.array_equal(pa, pb), 'infectee lists'
    # an inline block is filled by rank: no hole before a used slot, and the overflow list starts only when it is full
    used = (ia >= 0).sum(axis=1)
    assert np.array_equal(ia >= 0, np.arange(eng.INLINE_INFECTEES)[None, :] < used[:, None]), 'inline infectee slots are filled in rank order'
    assert np.all(used[fa >= 0] == eng.INLINE_INFECTEES), 'an overflow list beside a block that is not full'


def _run_and_compare(variables, ages, seed, days, interventions=None, chunk=None, ipc=None, **context_kw):
    if ipc is not None and variables['hospital_beds'] == 0 and dict(ipc).get('in_icu', 0) > 0:
        # people bound for ICU and no hospital beds: the reference does not construct (AssertionError out of Context.__init__,
        # DESIGN.md "Initial condition"), neither engine may -- unless the shortened walk leaves no ICU slot; then go on
        # without the ICU patients
        import par_backend
        outcomes = []
        for kw in (dict(), dict(engine_factory=par_backend.par_engine_factory)):
            try:
                simulation.make_context(variables, age_counts=ages, seed=seed, interventions=interventions, ipc=ipc, **kw, **context_kw)
                outcomes.append('constructed')
            except AssertionError as e:
                outcomes.append(str(e))
        assert outcomes[0] == outcomes[1], outcomes
        if outcomes[0] != 'constructed':
            ipc = dict(ipc, in_icu=0)
    gpu, cpu = _pair(variables, ages, seed, interventions, ipc, **context_kw)
    done = 0
    chunk = chunk or days
    from reina_model_amd.model import SimulationFailed
    while done < days:
        n = min(chunk, days - done)
        failed = []
        for ctx in (gpu, cpu):
            try:
                h = ctx.run(n)
            except SimulationFailed as e:  # the reference's own failure modes (e.g. 'Wrong state', quirk Q8)
                failed.append(str(e))
                h = None
            if ctx is gpu:
                hg = h
            else:
                hc = h
        if failed:
            assert len(failed) == 2 and failed[0] == failed[1], failed
            break
        if not np.array_equal(hg, hc):
            bad = np.nonzero((hg != hc).any(axis=1))[0][0]
            words = np.nonzero(hg[bad] != hc[bad])[0]
            raise AssertionError('first divergence at day %d, counter words %s gpu=%s cpu=%s' % (
                done + bad, words[:8], hg[bad][words[:8]], hc[bad][words[:8]]))
        done += n
    assert np.array_equal(gpu.engine.read_counters(), cpu.engine.read_counters())
    _assert_state_equal(gpu, cpu)
    return gpu, cpu


def _sharded_pair(v, ages, seed, G, attribution='exact', interventions=None, ipc=None, **context_kw):
    """G in-process shards on this GPU and the same on the CPU checker, cross-shard links `attribution` (sharding.py)"""
    import par_backend
    from reina_model_amd import sharding
    gm, cm = [], []
    gpu = [simulation.make_context(v, age_counts=ages, seed=seed, interventions=interventions, ipc=ipc,
                                   comm=sharding.InProcessComm(r, G, gm, attribution=attribution), **context_kw) for r in range(G)]
    cpu = [simulation.make_context(v, age_counts=ages, seed=seed, interventions=interventions, ipc=ipc,
                                   comm=sharding.InProcessComm(r, G, cm, attribution=attribution),
                                   engine_factory=par_backend.par_engine_factory, **context_kw) for r in range(G)]
    return gpu, cpu
