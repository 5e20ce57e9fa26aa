"""Every route that runs many members of one scenario (ensemble.run_ensemble, run_sweep, run_policy_ensemble, run_branches,
filtering.particle_filter with forecast and close, simulation.run_monte_carlo) and the two refusals of a foreign `group`, as
they were before the routes got one statement of how an ensemble is set up (reina_model_amd/ensemble.py: Setup, group_for,
check_shared_days, plan_once).  Every case is what the route returned -- crc32 of the history, of the summary's
words or of the frame's values --, every member's day, mobility factors and policy levels, the exact text of what it refused,
and what it built on the way: Contexts that made a plan (planners), the other Contexts (members), engine groups opened and
groups still open when the route returned.

The engines are oracle B's; the scenario is filter_util.small_scenario(20000), 3 members, 12 days.  ensemble_routes_util.py
holds the routes: tests/test_ensemble_routes_gpu.py runs the same ones on the device.

The expected results (tests/test_ensemble_routes.json) were recorded with this very file on commit 61e5866, the last one on
which every route wrote its set-up out: `python tests/test_ensemble_routes.py --record` rewrites the file from the code as it
stands, which is only ever right on a commit whose results are the ones to keep.  One figure is NOT the recorded one, and the
file's `comment` says so: run_monte_carlo made a planner per chunk of seeds (2 here) and makes one now."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]   # (for `python tests/test_ensemble_routes.py --record`)
import ensemble_routes_util as ru
import par_backend

WORDS = os.path.join(HERE, 'test_ensemble_routes.json')
COMMENT = ('recorded on commit 61e5866.  Since then one count has changed on purpose: run_monte_carlo makes its planner once, '
           'not once per chunk of seeds -- "planners" of the two monte_carlo cases is 2 here and 1 in the code as it stands '
           '(tests/test_ensemble_routes.py: PLANNERS_NOW).')
PLANNERS_NOW = {'monte_carlo': 1, 'monte_carlo_summary': 1}


def _case(name):
    return json.loads(json.dumps(ru.record(name, par_backend.par_engine_factory)))


@pytest.fixture(scope='module')
def expected():
    with open(WORDS) as f:
        return json.load(f)


@pytest.mark.parametrize('name', ru.CASES)
def test_every_route_gives_what_it_gave_before_the_set_up_was_stated_once(name, expected):
    want = dict(expected[name])
    if name in PLANNERS_NOW:
        assert want['built']['planners'] == 2
        want['built'] = dict(want['built'], planners=PLANNERS_NOW[name])
    assert _case(name) == want


def test_the_recorded_cases_are_worth_comparing_with(expected):
    """all names of this file and no others; the chunks are 2 and 1; the policy's members switch on different days; the filter
    resampled once, with a clone, in each of its cases; every refusal was raised, and no route leaves a group open but the
    filter, which closes it"""
    assert sorted(expected) == sorted(ru.CASES + ('comment',))
    assert expected['ensemble']['built'] == dict(planners=1, members=3, groups=2, open=0)
    assert len({tuple(m['policy_levels']) for m in expected['policy_ensemble']['members']}) == 3
    for name in ('filter', 'filter_snapshot'):
        f = expected[name]
        assert [len(set(a)) < 3 for a in f['ancestors']] in ([True, False], [False, True]), name
        assert f['built'] == dict(planners=1, members=3, groups=1, open=1) and f['open_after_close'] == 0, name
    for name, word in (('sweep_date', 'scenario 2 differs'), ('branches_policy_members', 'cannot be combined'),
                       ('foreign_group_plan', 'run_group_plan: `group` is not')):
        assert expected[name]['error'][0] == 'ValueError' and word in expected[name]['error'][1], name
    for name in ru.CASES:
        assert name.startswith('filter') or expected[name]['built']['open'] == 0, name


if __name__ == '__main__':
    if '--record' in sys.argv:
        out = {name: _case(name) for name in ru.CASES}
        out['comment'] = COMMENT
        with open(WORDS, 'w') as f:
            json.dump(out, f, separators=(',', ':'), sort_keys=True)
            f.write('\n')
