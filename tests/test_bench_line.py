"""The bench line's roofline object (bench.roofline_obj) on recorded numbers, no GPU: what round 4's verdict asked of it -- no
per-kernel fraction of the HBM peak above 1 under a name that says "fraction", the bytes actually moved beside the algorithmic
ones, the VALU-issue figures, a bound per regime, and the random-access bound of k_hosp_install."""
import json
import os

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _res(n_agents, day_us, k_day_us, install_us, infected, contacts, new_inf):
    return dict(dt=day_us * 1e-6 * 365, n_local=n_agents, rccl_world=None,
                prof={'k_open': (0.0133 * 23, 23), 'k_day': (k_day_us * 1e-3 * 23, 23), 'k_hosp_install': (install_us * 1e-3 * 23, 23)},
                stats=dict(infected_on_scan_days=infected, mean_infected=infected, contacts_per_day=contacts, contacts_on_scan_days=contacts,
                           new_infections_per_day=new_inf, removed_per_day=new_inf, final_all_infected=1, peak_infected=1))


def test_roofline_object_says_what_bounds_the_engine(monkeypatch):
    # the 2e8-agent year of round 5's collection: k_day 97.8 us for 841.6 MB of algorithmic bytes = 1.075 x the HBM peak
    moved = {'k_day': 323_000_000, 'k_hosp_install': 68_000_000}
    util = {'k_day': dict(valu_mean_day=0.5172, valu_peak_day=0.594, waiting_mean_day=0.52, waiting_peak_day=0.51),
            'k_hosp_install': dict(valu_mean_day=0.242, valu_peak_day=0.203, waiting_mean_day=0.75, waiting_peak_day=0.77)}
    monkeypatch.setattr(bench, 'traffic_for', lambda key: (406_277_956, moved, util, 'test'))
    r = bench.roofline_obj(200_000_000, _res(200_000_000, 168.0, 97.8, 44.1, 3.0e6, 7.8e6, 1.18e5), 365, 16, '200000000')
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-4
    text = json.dumps(r)
    assert 'frac_of_hbm_peak' not in text                      # (the name that could not be a fraction is gone)
    kd = r['kernels']['k_day']
    assert kd['vs_hot_word_streamer'] > 1.0                    # ... the comparison with a streamer may exceed 1, and says what it is
    assert 0.0 < kd['moved'] < 1.0 and 0.0 < r['moved']['frac'] < 1.0 and r['moved']['frac'] < r['frac']
    assert r['traffic'] == r['moved']['bytes_per_day'] and r['wasted'] == round(r['moved']['bytes_per_day'] / r['model_bytes_per_day'], 3)
    assert r['valu']['k_day'] == {'mean_day': 0.5172, 'peak_day': 0.594} and 'k_hosp_install' in r['valu']
    assert set(r['bound_by_regime']) == {'quiet_day', 'peak_day'} and 'latency' in r['bound_by_regime']['quiet_day'] and 'valu' in r['bound_by_regime']['peak_day']
    ra = r['kernels']['k_hosp_install']['random_access']
    assert 0.5 < ra['frac'] <= 1.05 and ra['floor_us'] > 20      # (at 2e8 agents the launch runs close to the chip's random-access rate)


def test_no_traffic_means_no_moved_figure():
    r = bench.roofline_obj(1_685_983, _res(1_685_983, 40.0, 14.0, 12.0, 500.0, 2000.0, 50.0), 365, 16, None)
    assert r['moved'] is None and r['traffic'] is None and r['wasted'] is None and r['valu'] is None
    assert 'vs_hot_word_streamer' in r['kernels']['k_day'] and 'moved' not in r['kernels']['k_day']


def test_recorded_bench_line_of_the_round_carries_the_new_fields():
    """profiles/r05_bench.json (the line of the final binary, collected on the GPU box): every full_scenario entry and the headline
    carry moved / valu / bound_by_regime, no fraction above 1 under the names that are fractions"""
    b = json.load(open(os.path.join(ROOT, 'profiles', 'r05_bench.json')))
    lines = [b['roofline']] + [fs['roofline'] for fs in b['full_scenario'].values()]
    assert len(lines) == 5
    for r in lines:
        assert r['moved'] and 0 < r['moved']['frac'] < 1 and r['valu'] and r['bound_by_regime'] and 0 < r['frac'] < 1
        for k, ent in r['kernels'].items():
            assert 'frac_of_hbm_peak' not in ent
            if 'moved' in ent:
                assert 0 < ent['moved'] < 1, (k, ent)
    assert b['metric'] == 'agent-days/sec' and b['dtype'] == 'u32' and 'cpu_baseline' in b and b['vs_baseline'] is None


def test_the_instrument_is_thin_in_a_short_window():
    """A timestamped dispatch costs wall time (5.5-8 us: tools/window_probe.py), and the round driver's window is 20 days long: a run of
    16-63 days times one kernel every other day (stride 8: each of the four phases twice or three times in 20 days), a longer one every
    fourth day, only the shortest every day -- and any `stride` consecutive days still time every kind once."""
    assert bench.stride_for(20, 0) == 8 and bench.stride_for(64, 0) == 16 and bench.stride_for(365, 0) == 16 and bench.stride_for(5, 0) == 4
    assert bench.stride_for(20, 12) == 12 and bench.stride_for(365, 2) == 4   # (--time-every: multiples of four, at least four)
    for steps, warmup in ((20, 5), (30, 0), (365, 5)):
        stride = bench.stride_for(steps, 0)
        phases = {0: 0, stride // 4: 0, stride // 2: 0, stride // 2 + stride // 4: 0}   # (reina_hip.hip: profiled_kind)
        for day in range(warmup, warmup + steps):
            if day % stride in phases:
                phases[day % stride] += 1
        assert min(phases.values()) >= 1, (steps, phases)
        if steps == 20:
            assert sum(phases.values()) <= 10 and min(phases.values()) >= 2   # (15 of them until round 5's last day)
    # the trace's per-kernel means ride on the line beside the HIP-event means when profiles/traffic.json matches the binary
    r = bench.roofline_obj(1_685_983, _res(1_685_983, 40.0, 14.0, 12.0, 500.0, 2000.0, 50.0), 365, 16, None)
    assert 'kernel_us_per_day_trace' not in r and 'timestamped dispatches' in r['kernel_timing']


def test_line_fits():
    """Round 5's line was 24.5 KB and the round driver could not parse it (BENCH_r05.json: parsed null).  The printed line is a
    digest of at most 8000 bytes -- contract fields, roofline (headline + per-size table), cpu_baseline, ensemble --, the full
    objects go to profiles/bench_detail.json."""
    full = json.load(open(os.path.join(ROOT, 'profiles', 'r05_bench_driver_window.json')))   # the 24.5 KB object of round 5
    line = bench.compact_line(full)
    text = json.dumps(line, separators=(',', ':'))
    assert len(text) < bench.LINE_LIMIT <= 8000 and '\n' not in text
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in line, k
    r = line['roofline']
    assert set(('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic')) <= set(r) and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-4
    assert set(r['full_scenario_365d']) == {'hus', '50000000', '100000000', '200000000'}
    big = r['full_scenario_365d']['100000000']
    assert big['k_day']['trace_us'] and big['k_day']['pmc_bytes'] and 0 < big['moved_frac'] < big['frac'] < 1
    c = line['cpu_baseline']
    assert set(('value', 'unit', 'cores', 'kind', 'sample')) <= set(c) and c['kind'] == 'port' and c['all_cores']['cores'] >= 1
    assert line['ensemble']['value'] > 0 and 'model' not in line['config']
    # a line that still does not fit sheds its widest optional parts instead of growing
    fat = json.loads(json.dumps(full))
    for k in list(fat['full_scenario']):
        for j in range(40):
            fat['full_scenario']['%s_%d' % (k, j)] = fat['full_scenario'][k]
    thin = bench.compact_line(fat)
    assert len(json.dumps(thin, separators=(',', ':'))) < bench.LINE_LIMIT and thin.get('truncated') and 'cpu_baseline' in thin


def test_recorded_line_of_this_round_parses_and_fits():
    """profiles/r06_bench_line.json holds the line exactly as bench.py printed it on the GPU box (when it has been collected)"""
    p = os.path.join(ROOT, 'profiles', 'r06_bench_line.json')
    if not os.path.exists(p):
        import pytest
        pytest.skip('no recorded line yet')
    text = open(p).read().strip()
    assert len(text) < 8000 and len(text.splitlines()) == 1
    line = json.loads(text)
    assert line['roofline']['frac'] > 0 and line['cpu_baseline']['value'] > 0 and line['dtype'] == 'u32'


def test_a_multi_gpu_line_fits_too():
    """`bench.py --gpus N` adds `large`, `strong` (with the other attribution mode beside it) and a distributed `ensemble` to the object:
    the digest keeps them under the same cap (verdict r05 item 9: "keep the --gpus 8 line under item 1's size cap too")"""
    # (the full object of round 6's recorded run; profiles/bench_detail.json is rewritten by every bench.py run)
    full = json.load(open(os.path.join(ROOT, 'profiles', 'r06_bench_detail.json')))
    fs = full['full_scenario']['100000000']
    out = {k: v for k, v in full.items() if k not in ('full_scenario', 'cpu_baseline', 'value_warm', 'ms_per_step_warm', 'headline_is')}
    out['n_gpus'] = 8
    out['config'] = dict(out['config'], attribution='mirror', rccl_world=8, collective='ncclAllReduce queued on the day stream (own RCCL communicator)',
                         parallelism='agents sharded x8, one RCCL all-reduce per day (infection pressure + the shards\' bed / ICU event maps)')
    roof = json.loads(json.dumps(fs['roofline']))
    roof['kernels']['k_remote'] = dict(avg_launch_us=12.9, timed_launches=23)
    roof['kernels']['collective'] = dict(avg_launch_us=31.0, timed_launches=23)
    out['large'] = dict(workload='synthetic 400000000 agents (50000000 per GPU, BASELINE configs[3] shape), default scenario scaled, 365 days',
                        value=1.0e12, unit='agent-days/s', ms_per_step=0.146, roofline=roof, final_all_infected=1)
    out['strong'] = dict(workload='synthetic 100000000 agents in total', scaling='strong', attribution='mirror', value=7.0e11, unit='agent-days/s',
                         ms_per_step=0.052, rccl_world=8, roofline=roof, final_all_infected=1, expect='x' * 700,
                         exact=dict(value=6.0e11, ms_per_step=0.061, kernels={'k_day': 50.0}, exchange_segment_fill={'peak_records': 1, 'capacity': 2}))
    line = bench.compact_line(out)
    text = json.dumps(line, separators=(',', ':'))
    assert len(text) < bench.LINE_LIMIT and not line.get('truncated')
    assert line['n_gpus'] == 8 and line['config']['attribution'] == 'mirror' and line['config']['rccl_world'] == 8
    assert line['large']['value'] == 1.0e12 and line['large']['kernel_us']['collective'] == 31.0 and line['large']['roofline']['frac'] > 0
    assert line['strong']['exact']['value'] == 6.0e11 and line['strong']['scaling'] == 'strong' and 'cpu_baseline' not in line


def test_dump_outputs_writes_float64_arrays_under_the_cap(tmp_path):
    """`bench.py --dump-outputs DIR`: the timed run's history and the counters of its last day as float64 .npy files, at most
    64 MB in all even for the longest run the engine allows (MAX_DAYS - 1 timed days)"""
    import numpy as np
    from reina_model_amd import engine as eng
    W = eng.COUNTER_WORDS
    hist = (np.arange(20 * W, dtype=np.int64) % 2**31).astype(np.int32).reshape(20, W)
    final = np.arange(W, dtype=np.int32) - 7
    bench.dump_outputs(str(tmp_path / 'a'), dict(history=hist, final_counters=final, first_day=5))
    h = np.load(tmp_path / 'a' / 'history.npy')
    assert h.dtype == np.float64 and np.array_equal(h, hist)
    assert np.array_equal(np.load(tmp_path / 'a' / 'history_days.npy'), np.arange(5, 25))
    f = np.load(tmp_path / 'a' / 'final_counters.npy')
    assert f.dtype == np.float64 and np.array_equal(f, final)
    longest = np.ones((eng.MAX_DAYS - 1, W), dtype=np.int32)
    bench.dump_outputs(str(tmp_path / 'b'), dict(history=longest, final_counters=final, first_day=1))
    assert sum(p.stat().st_size for p in (tmp_path / 'b').iterdir()) <= 64_000_000
    assert np.load(tmp_path / 'b' / 'history.npy').shape == longest.shape
