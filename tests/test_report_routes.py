"""The course and vaccination reports through every route by which a report of a log is taken, as they were before the four
reports got one statement of those routes (reina_model_amd/reports.py: the report kind and its three routes): the single
route, the list route, and the refusals of both.  tests/test_reports_words.py holds the same for the log and lineage reports;
its file and cases stay as they are.  Every case is the sha256 of the report's words and its scalars by name, or the type and
text of the exception it raised.

The run is oracle B's: vacc_util.vaccination_scenario() with a log and a course, seeds 3 and 4, 60 days.

The expected results (tests/test_report_routes.json) were recorded with this very file on commit 88d6790, the last one on which
txlog.py, lineage.py, course.py, vaccination.py, ensemble.py and filtering.py each wrote their routes out: `python
tests/test_report_routes.py --record` rewrites the file from the code as it stands, which is only ever right on a commit whose
words are the ones to keep."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]   # (for `python tests/test_report_routes.py --record`)
import par_backend
import tx_util
import vacc_util
from reina_model_amd import course as crs, ensemble, simulation, vaccination as vac

WORDS = os.path.join(HERE, 'test_report_routes.json')
DAYS = 60


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _result(fn):
    """what a call gave: a report (or a list of them) as hash and scalars, or the exception it raised"""
    try:
        r = fn()
    except Exception as e:        # noqa: BLE001  (the refusals are cases too)
        return dict(error=[type(e).__name__, str(e)])
    if isinstance(r, list):
        return [_result(lambda x=x: x) for x in r]
    module = {crs.CourseReport: crs, vac.VaccinationReport: vac}[type(r)]
    out = dict(words=_sha(r.words), scalars={name: int(getattr(r, name)) for name in module.SCALAR_NAMES}, n_days=int(r.n_days),
               n_groups=int(r.n_groups), group_labels=r.group_labels, start_date=str(r.start_date))
    if module is vac:
        out['group_sizes'] = [int(x) for x in r.group_sizes]
        out['by_status'] = [int(x) for x in r.outcome[:, :, 0].sum(axis=1)]
    return out


def _context(seed, **kw):
    v, ages = vacc_util.vaccination_scenario()
    return simulation.make_context(v, age_counts=ages, seed=seed, ipc='auto', engine_factory=par_backend.par_engine_factory, **kw)


@functools.lru_cache(maxsize=None)
def _runs():
    """two 60-day runs in host memory with a log and a course; a Context with a log alone and one with neither (they are only
    ever refused, so they run no day)"""
    a, b = _context(3, txlog=True, course=True), _context(4, txlog=True, course=True)
    a.run(DAYS)
    b.run(DAYS)
    return a, b, _context(3, txlog=True), _context(3)


FOUR = dict(log_reports=ensemble.log_reports, lineage_reports=ensemble.lineage_reports, course_reports=ensemble.course_reports,
            vaccination_reports=ensemble.vaccination_reports)


def _run(route):
    a, b, log_only, plain = _runs()
    course, log = a.course_log, a.transmission_log
    fine = tx_util.groups('fine')
    return _result({'course': course.report, 'course_40_days': lambda: course.report(n_days=40), 'course_fine': lambda: course.report(fine),
                    'vaccination': log.vaccination_report, 'vaccination_40_days': lambda: log.vaccination_report(n_days=40),
                    'vaccination_fine': lambda: log.vaccination_report(fine),
                    'ensemble_course': lambda: ensemble.course_reports([a, b]),
                    'ensemble_vaccination': lambda: ensemble.vaccination_reports([a, b])}[route])


RUN = ('course', 'course_40_days', 'course_fine', 'vaccination', 'vaccination_40_days', 'vaccination_fine', 'ensemble_course',
       'ensemble_vaccination')


def _refusal(name):
    a, b, log_only, plain = _runs()
    course, log = a.course_log, a.transmission_log
    if name == 'mixed_course':
        routes = dict(first=lambda: ensemble.course_reports([a, log_only]), last=lambda: ensemble.course_reports([log_only, a]))
    elif name == 'no_log':
        routes = {what: functools.partial(fn, [a, plain]) for what, fn in FOUR.items()}
        routes.update({what + '_alone': functools.partial(fn, [plain]) for what, fn in FOUR.items()})
    elif name.startswith('n_days_'):
        value = int(name.rpartition('_')[2])
        routes = dict(course=lambda: course.report(n_days=value), vaccination=lambda: log.vaccination_report(n_days=value),
                      ensemble_course=lambda: ensemble.course_reports([a, b], n_days=value),
                      ensemble_vaccination=lambda: ensemble.vaccination_reports([a, b], n_days=value))
    else:
        kind, _, value = name.rpartition('_')
        table = tx_util.groups()[:int(value)] if kind == 'ages' else np.full(tx_util.NR_AGES, int(value))
        routes = dict(course=lambda: course.report(table), vaccination=lambda: log.vaccination_report(table),
                      ensemble_course=lambda: ensemble.course_reports([a, b], table),
                      ensemble_vaccination=lambda: ensemble.vaccination_reports([a, b], table))
    return {route: _result(fn) for route, fn in routes.items()}


REFUSALS = ('mixed_course', 'no_log', 'n_days_0', 'n_days_4097', 'ages_50', 'group_16')

CASES = {'run-' + r: functools.partial(_run, r) for r in RUN}
CASES.update({'refusal-' + r: functools.partial(_refusal, r) for r in REFUSALS})


@pytest.fixture(scope='module')
def expected():
    with open(WORDS) as f:
        return json.load(f)


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_route_gives_what_it_gave_before_the_routes_were_stated_once(name, expected):
    assert json.loads(json.dumps(CASES[name]())) == expected[name]


def _leaves(x):
    if isinstance(x, list):
        for y in x:
            yield from _leaves(y)
    elif 'scalars' in x or 'error' in x:
        yield x
    else:
        for y in x.values():
            yield from _leaves(y)


def test_the_recorded_cases_are_worth_comparing_with(expected):
    """the recorded run has breakthrough infections, protected ones among them, admissions and ICU admissions; every refusal
    was raised (an age table shorter than the population by the vaccination report only: course.report_numpy on host copies
    takes the ages it is given, as txlog.report_numpy does); all names of this file and no others"""
    assert sorted(expected) == sorted(CASES)
    v, c = expected['run-vaccination'], expected['run-course']
    assert v['scalars']['vaccinated_infected'] > 0
    assert v['by_status'][vac.PROTECTED] > 0
    assert c['scalars']['with_admission'] > 0
    assert c['scalars']['with_icu'] > 0
    for name in RUN:
        assert all('scalars' in x for x in _leaves(expected['run-' + name])), name
    for name in REFUSALS:
        errors = [x for x in _leaves(expected['refusal-' + name]) if 'error' in x]
        assert errors and all(e['error'][0] == 'ValueError' for e in errors), name
        assert len(errors) == len(list(_leaves(expected['refusal-' + name]))) or name == 'ages_50', name


if __name__ == '__main__':
    if '--record' in sys.argv:
        with open(WORDS, 'w') as f:
            json.dump({name: CASES[name]() for name in sorted(CASES)}, f, separators=(',', ':'), sort_keys=True)
            f.write('\n')
