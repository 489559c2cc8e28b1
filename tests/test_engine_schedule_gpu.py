"""The engine's launch schedule is its behaviour: ``libsegmi.so`` computes a function of the ``ops.*`` calls the engine
makes, their operands, the stream each is issued on and the ordering edges between them.  Each configuration of
tests/golden/make_engine_schedule_goldens.py (two training steps and an eval forward) is traced again and must equal,
event for event, the schedule recorded in tests/golden/engine_schedule_parent.json.
"""
import json

import pytest

pytestmark = pytest.mark.gpu

from tests.golden import make_engine_schedule_goldens as gen  # noqa: E402
from tests.helpers import engine_trace  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return engine_trace.decode(json.loads(gen.GOLDEN.read_text()))


def test_the_recorded_schedules_contain_every_launch_form(recorded):
    assert sorted(recorded) == sorted(gen.CONFIGS)
    assert gen.census_missing(recorded) == []


@pytest.mark.parametrize("name", list(gen.CONFIGS), ids=[n.replace(" ", "_") for n in gen.CONFIGS])
def test_engine_issues_the_recorded_schedule(recorded, name):
    # through JSON, as the recorded one went: tuples and lists are one thing there
    got = json.loads(json.dumps(gen.run_config(gen.CONFIGS[name])))
    difference = engine_trace.first_difference(got, recorded[name])
    if difference:
        print(difference)
    assert difference is None, difference
