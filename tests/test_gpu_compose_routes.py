"""
The native entry points every model family calls, pass by pass, against the committed record (tests/golden/compose_routes.json, written
by tools/compose_routes.py --write): a change in layers.Compose's dispatch that costs or saves a launch shows here.  Needs a real MI355X.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('compose_routes', os.path.join(ROOT, 'tools', 'compose_routes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(TOOL.GOLDEN) as _f:
    WANT = json.load(_f)


def test_the_record_covers_the_cases():
    assert sorted(WANT) == sorted(TOOL.cases())


@pytest.mark.parametrize('case', list(TOOL.cases()))
def test_models_call_the_recorded_entry_points(pkg, case):
    got = TOOL.names(TOOL.record(pkg, case))
    assert list(got) == list(TOOL.PHASES)
    for phase in TOOL.PHASES:
        assert got[phase].split() == WANT[case][phase].split(), '%s / %s' % (case, phase)
