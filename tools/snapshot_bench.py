"""Snapshot throughput on one MI355X: prints ONE JSON line.

Cases: 1e8 agents on day 120 of the default scenario (pack, unpack), HUS on day 200 (pack, unpack), a 128-member HUS fork
(reina_group_snap_unpack) against 128 single reina_snap_unpack calls.  Times are HIP events around the library calls
(pack includes its count + scan launches and the waits reina_snap_measure / reina_snap_pack do; unpack includes the header
read-back).  Bytes are computed from the shapes and the recorded-agent counts; GB/s against 6.3 TB/s achievable / 8 TB/s
spec HBM bandwidth.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/snapshot_bench.py`.

    python tools/snapshot_bench.py [--agents 100000000] [--members 128] [--reps 5]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from reina_model_amd import datasets, engine as eng, simulation, snapshot as snapmod  # noqa: E402
from reina_model_amd.variables import VARIABLE_DEFAULTS  # noqa: E402

ACHIEVABLE, SPEC = 6.3e12, 8.0e12
AGENT_BYTES = 4 + 4 * eng.COLD_WORDS + 4 * eng.INLINE_INFECTEES   # words an unpack writes per agent (+ 2 bits)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return float(np.median(out)), float(min(out))


def bw(nbytes, ms):
    return dict(bytes=int(nbytes), gbs=nbytes / (ms * 1e-3) / 1e9, of_achievable=nbytes / (ms * 1e-3) / ACHIEVABLE,
                of_spec=nbytes / (ms * 1e-3) / SPEC)


def pack_unpack_case(v, ages, days, seed, reps):
    a = simulation.make_context(v, age_counts=ages, seed=seed)
    a.run(days, record_history=False)
    a.synchronize()
    snap = a.snapshot()
    h = snap.header
    n = a.total_people
    rec = h['n_base']
    pack_ms, pack_min = timed(lambda: a.snapshot(), reps)
    b = simulation.make_context(v, age_counts=ages, seed=seed)
    f = b.engine.snap_f

    def unpack():
        b.engine._check(f['snap_unpack'](b.engine._h, snap.image.data_ptr(), b.engine.alloc.stream()), 'snap_unpack')
    unpack_ms, unpack_min = timed(unpack, reps)
    # count: hot words + the slot-0 sector of every recorded agent; pack adds the cold records and slots read and both streams
    # written; unpack reads the image and writes every agent's words + the two bit planes
    count_bytes = 4 * n + 32 * rec
    pack_bytes = count_bytes + 4 * n + 32 * rec + 32 * h['n_slot'] + snap.nbytes
    unpack_bytes = snap.nbytes + AGENT_BYTES * n + 2 * eng.bits_words(n) * 4
    res = dict(agents=n, day=days, recorded=rec, with_slots=h['n_slot'], snapshot_bytes=snap.nbytes,
               dense_bytes=AGENT_BYTES * n, pack_ms=pack_ms, pack_ms_min=pack_min, unpack_ms=unpack_ms, unpack_ms_min=unpack_min,
               pack=bw(pack_bytes, pack_ms), unpack=bw(unpack_bytes, unpack_ms))
    del a, b
    return res, snap


def fork_case(v, ages, snap, members, reps):
    ctxs = [simulation.make_context(v, age_counts=ages, seed=100 + k) for k in range(members)]
    group = eng.EngineGroup([c.engine for c in ctxs])
    f = ctxs[0].engine.snap_f
    e0 = ctxs[0].engine

    def fork():
        e0._check(f['group_snap_unpack'](group._h, snap.image.data_ptr(), e0.alloc.stream()), 'group_snap_unpack')

    def singles():
        for c in ctxs:
            c.engine._check(f['snap_unpack'](c.engine._h, snap.image.data_ptr(), c.engine.alloc.stream()), 'snap_unpack')
    fork_ms, fork_min = timed(fork, reps)
    single_ms, single_min = timed(singles, reps)
    n = ctxs[0].total_people
    written = members * (AGENT_BYTES * n + 2 * eng.bits_words(n) * 4)
    group.close()
    return dict(members=members, agents=n, fork_ms=fork_ms, fork_ms_min=fork_min, singles_ms=single_ms,
                singles_ms_min=single_min, fork=bw(written + snap.nbytes, fork_ms), singles=bw(written + members * snap.nbytes, single_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=100_000_000)
    ap.add_argument('--members', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    v = copy.deepcopy(VARIABLE_DEFAULTS)
    out = dict(tool='snapshot_bench', achievable_tbs=ACHIEVABLE / 1e12, spec_tbs=SPEC / 1e12)
    out['hus_day200'], hus_snap = pack_unpack_case(v, datasets.get_population_for_area('HUS'), 200, 1, args.reps)
    out['hus_fork'] = fork_case(v, datasets.get_population_for_area('HUS'), hus_snap, args.members, args.reps)
    del hus_snap
    torch.cuda.empty_cache()
    if args.agents:
        out['big_day120'], _ = pack_unpack_case(v, datasets.scaled_population(args.agents), 120, 1, args.reps)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
