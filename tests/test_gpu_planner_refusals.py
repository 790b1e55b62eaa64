"""The refusals of the lookahead queries (TBX_QUERY_LOOKAHEAD .. _ACT, include/toybox_amd.h), held to a recording byte for byte.

tests/golden/planner_refusals.json holds, per game, what the library of the commit before the planners' host code was put behind
one shared-row check answered to a fixed list of refused shared rows (scripts/record_planner_refusals.py has the list and says how
it is recorded -- from the commit before a change, never from the changed library): single faults, and rows with two faults, where
the message says which of a query's checks comes first.  Here every row is asked again: the same code, the same message.  Nothing
is launched for a refused row, so afterwards the counters stand where one valid query of each kind left them, and a valid query of
each kind answers what it answered before."""
import json
import os

import numpy as np
import pytest

from toybox_amd import ToyboxAmdError, _abi
from toybox_amd.engine import Engine

pytestmark = pytest.mark.gpu

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
ENVS = 8
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner_refusals.json")
PREFIX = "toybox_amd error %d: "
COUNTERS = (_abi.OPT_SEARCH_CHUNKS, _abi.OPT_SAMPLE_CHUNKS, _abi.OPT_SEARCH_SAMPLES_CHUNKS, _abi.OPT_SEARCH_SAMPLES_LAUNCHES, _abi.OPT_BEAM_RANGES,
            _abi.OPT_BEAM_SAMPLES_RANGES, _abi.OPT_BEAM_SAMPLES_CHUNKS, _abi.OPT_EVOLVE_RANGES)
TAIL = [-1, 0, 0, 0, 0]
# one valid shared row of each kind, small: {frames, hold, ...}
VALID = {_abi.QUERY_LOOKAHEAD: [8, 2], _abi.QUERY_LOOKAHEAD_ALL: [8, 2], _abi.QUERY_LOOKAHEAD_PLAN: [8, 2, 2, 3], _abi.QUERY_LOOKAHEAD_SEARCH: [8, 2, 2, 1],
         _abi.QUERY_LOOKAHEAD_SAMPLES: [8, 2, 3, 5], _abi.QUERY_LOOKAHEAD_SEARCH_SAMPLES: [8, 2, 2, 0] + TAIL + [3, 5], _abi.QUERY_LOOKAHEAD_BEAM: [8, 2, 3, 0] + TAIL + [2],
         _abi.QUERY_LOOKAHEAD_BEAM_SAMPLES: [8, 2, 3, 1] + TAIL + [2, 2, 5], _abi.QUERY_LOOKAHEAD_EVOLVE: [8, 2, 3, 0] + TAIL + [4, 1, 2, 7, 64, -1],
         _abi.QUERY_LOOKAHEAD_ACT: [_abi.QUERY_LOOKAHEAD_BEAM, 8, 2, 3, 0] + TAIL + [2]}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_covers_every_game_and_query(recorded):
    assert sorted(recorded) == sorted(GAMES)
    for game in GAMES:
        assert {r["query"] for r in recorded[game]} == set(VALID), game
        assert all(r["code"] == _abi.E_INVALID and r["message"] for r in recorded[game]), game


@pytest.mark.parametrize("game", GAMES)
def test_refusals_are_the_recorded_ones(game, recorded, hip_lib):
    e = Engine(game, ENVS, lib=hip_lib)
    try:
        e.seed(1234)
        e.new_game()
        answers = {q: e.reduce(q, row) for q, row in VALID.items()}
        counters = [e.get_option(o) for o in COUNTERS]
        assert all(c >= 1 for c in counters), counters
        for r in recorded[game]:
            args = np.tile(np.asarray(r["args"], np.float64), (ENVS, 1)) if r["per_env"] else r["args"]
            with pytest.raises(ToyboxAmdError) as ei:
                e.reduce(r["query"], args)
            assert ei.value.code == r["code"], (r, str(ei.value))
            assert str(ei.value) == PREFIX % r["code"] + r["message"], (r, str(ei.value))
        assert [e.get_option(o) for o in COUNTERS] == counters, "a refusal moved a counter"
        for q, row in VALID.items():
            assert np.array_equal(e.reduce(q, row), answers[q]), "query %d answers differently after the refusals" % q
        assert [e.get_option(o) for o in COUNTERS] == counters
    finally:
        e.close()
