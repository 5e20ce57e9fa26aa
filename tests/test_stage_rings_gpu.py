"""The two users of the pinned staging ring (csrc/k_common.inc: StageRing) under reuse: the engine's table uploads and the
summary's head, each asked for slots back to back.  Neither test can force the ring to grow to its cap or to wait for slot 0:
which of its three paths a call takes -- a slot whose copy has left it, a new slot, the wait -- depends on how far the GPU has
got.  They hold the results whichever path is taken."""
import numpy as np
import pytest

import summary_util as su
from filter_util import small_scenario
from reina_model_amd import simulation, summary as sm

pytestmark = pytest.mark.gpu

DAYS, MORE, UPLOADS = 200, 5, 40      # (the engine's ring holds 32 slots)


def test_the_table_ring_asked_for_more_than_its_slots_delivers_the_last_table():
    """200 days queued with nothing read back, then 40 uploads back to back that alternate two tables -- more than the ring's
    32 slots while the earlier ones may still be busy --, then 5 days: state and history word for word those of a Context that
    ran the same 205 days and was given the last table alone at day 200."""
    v, ages = small_scenario(20000)
    a, b = (simulation.make_context(v, age_counts=ages, seed=5) for _ in range(2))
    for ctx in (a, b):
        assert ctx.run(DAYS, record_history=False) is None
    nrc, count, thr, meta, mask, ranges = a._packed_tables()
    tables = [(nrc, count, thr, meta, mask, ranges), (nrc * np.float32(0.5), count, thr, meta, mask, ranges)]
    assert not np.array_equal(tables[0][0], tables[1][0])
    for k in range(UPLOADS):
        a.engine.upload_contact_tables(*tables[k % 2])
    b.engine.upload_contact_tables(*tables[(UPLOADS - 1) % 2])
    ha, hb = a.run(MORE), b.run(MORE)
    assert np.array_equal(ha, hb)
    assert np.array_equal(a.engine.read_counters(), b.engine.read_counters())
    for name in ('hot', 'infector', 'n_infected'):
        assert bool((a.engine.tensors[name] == b.engine.tensors[name]).all()), name
    # ... and the last table is not the one the days before ran on: with it the five days differ
    c = simulation.make_context(v, age_counts=ages, seed=5)
    c.run(DAYS, record_history=False)
    assert not np.array_equal(c.run(MORE), ha)


def test_the_summary_ring_serves_twelve_summaries_back_to_back():
    """twelve summaries of one device history of 5 members x 9 days with twelve different rank sets -- more than the ring's
    8 slots --, each equal to the specification's"""
    import torch
    K, days, nr_ages = 5, 9, 101
    h = su.history(K, days, nr_ages, 'random', seed=2)
    dev = torch.from_numpy(h).to('cuda:0')
    assert sm.library() is not None
    specs = [sm.SummarySpec(tuple(((k + j) % 12) / 11.0 for j in range(1 + k % 4))) for k in range(12)]
    assert len({tuple(sm.Layout(s, K, days, nr_ages).ranks.tolist()) for s in specs}) == 12
    got = [sm.summarise(dev, nr_ages, s) for s in specs]
    for g, s in zip(got, specs):
        su.assert_words(g.words, sm.summarise_numpy(h, nr_ages, s), g.layout)
    assert np.array_equal(dev.cpu().numpy(), h)
