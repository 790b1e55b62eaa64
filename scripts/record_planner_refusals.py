#!/usr/bin/env python3
"""Record what the lookahead queries (TBX_QUERY_LOOKAHEAD .. _ACT, include/toybox_amd.h) answer to a fixed list of refused shared
rows: per game and query {args, per_env, code, message} into tests/golden/planner_refusals.json, which
tests/test_gpu_planner_refusals.py replays.  The list pins WHICH check of a query speaks first, so a change to the host code in
front of the planners is held to the recorded library byte for byte.

Run it against the library of the commit BEFORE such a change (built in a second checkout), never against the changed one:

    python scripts/record_planner_refusals.py --lib /path/to/parent/toybox_amd/csrc/libtoybox_amd.so [--out tests/golden/planner_refusals.json]

Needs a GPU (the library makes its engines on device 0).  Every row of the list must be refused: asserted.

The rows: the single faults of the refusal tests of tests/test_gpu_lookahead.py, _search.py, _samples.py, _search_samples.py,
_beam.py, _beam_samples.py and _evolve.py; the same rows of the five planners behind TBX_QUERY_LOOKAHEAD_ACT, and its own refusals
(unknown planner, too many arguments, per-env rows); and rows with TWO faults, where the message says which check comes first."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from toybox_amd import ToyboxAmdError, _abi  # noqa: E402
from toybox_amd.engine import Engine  # noqa: E402

GAMES = ("breakout", "space_invaders", "amidar", "gridworld")
ENVS = 8
LOOKAHEAD, ALL, PLAN, SEARCH, SAMPLES = _abi.QUERY_LOOKAHEAD, _abi.QUERY_LOOKAHEAD_ALL, _abi.QUERY_LOOKAHEAD_PLAN, _abi.QUERY_LOOKAHEAD_SEARCH, _abi.QUERY_LOOKAHEAD_SAMPLES
SEARCH_SAMPLES, BEAM, BEAM_SAMPLES = _abi.QUERY_LOOKAHEAD_SEARCH_SAMPLES, _abi.QUERY_LOOKAHEAD_BEAM, _abi.QUERY_LOOKAHEAD_BEAM_SAMPLES
EVOLVE, ACT = _abi.QUERY_LOOKAHEAD_EVOLVE, _abi.QUERY_LOOKAHEAD_ACT
PLANNERS = (SEARCH, SEARCH_SAMPLES, BEAM, BEAM_SAMPLES, EVOLVE)
MOST_ARGS = {SEARCH: 9, SEARCH_SAMPLES: 11, BEAM: 10, BEAM_SAMPLES: 12, EVOLVE: 15}
PREFIX = "toybox_amd error %d: "


def legal_count(lib, game):
    return lib.tbx_legal_actions(_abi.GAME_IDS[game], None, 0)


def refused_rows(game, L):
    """[(query, args, per_env)] -- the fixed list for one game of L legal actions"""
    top = _abi.PLAN_MAX_DEPTH[game]
    illegal = 2 if game == "breakout" else 17
    too_deep = {4: 7, 5: 6, 6: 5}[L]                         # the smallest depth with L^depth > TBX_LOOKAHEAD_MAX_PLANS
    cap = _abi.LOOKAHEAD_MAX_LEAVES // (L * 64 * L)
    tail = [-1, 0, 0, 0, 0]                                  # rest, seed_lo, seed_hi, t, env_offset
    head = [8, 1, 2, 0]
    nine = head + tail
    big = 2 ** 32
    single = {
        LOOKAHEAD: [[0], [1025], [8, 0], [8, 1, illegal], [8, 1, -1, illegal], [8, 1, -1, -1, 0, 0, 0, 0, 0], []],
        ALL: [[0], [1025], [8, 0], [8, 1, -1, illegal], [8, 1, -1, -1, 0, 0, 0, 0, 0], []],
        SEARCH: [[8, 1, 0], [8, 1, too_deep], [8, 1, 2, 2], [8, 1, 2, 0, illegal], [0], [1025], [8, 0], [8, 1, 1, 0, -1, 0, 0, 0, 0, 0], []],
        PLAN: [[8, 1, 2, L * L], [8, 1, 2, -1], [8, 1, 0, 1], [8, 1, top + 1, 0], [8, 1, -1], [8, 1, 2, 0, illegal], [0], [1025], [8, 0],
               [8, 1, 1, 0, -1, 0, 0, 0, 0, 0], []],
        SAMPLES: [[8, 1, 0], [8, 1, 4097], [8, 1, 4, -1], [8, 1, 1, big], [8, 1, 4, big - 3], [8, 1, 2, 0, illegal], [0], [1025], [8, 0],
                  [8, 1, 1, 0, -1, 0, 0, 0, 0, 0], []],
        SEARCH_SAMPLES: [[0], [1025], [8, 0], [8, 1, 0], [8, 1, too_deep], [8, 1, 2, 2], [8, 1, 2, 0, illegal], nine + [0], nine + [4097],
                         [8, 1, too_deep - 1, 0] + tail + [64], nine + [2, -1], nine + [2, big], nine + [3, big - 2], nine + [2, 0, 0], []],
        BEAM: [[8, 1, 0], [8, 1, top + 1], [8, 1, 2, 2], [8, 1, 2, 0, illegal], [0], [1025], [8, 0], nine + [0], nine + [65], [8, 1, 1, 0] + tail + [1, 0], []],
        BEAM_SAMPLES: [[0], [1025], [8, 0], [8, 1, 0], [8, 1, top + 1], [8, 1, 2, 2], [8, 1, 2, 0, illegal], nine + [0], nine + [65], nine + [2, 0], nine + [2, 4097],
                       [8, 1, 5, 0] + tail + [64, cap + 1], [8, 1, top, 0] + tail + [64, cap + 1], nine + [2, 2, -1], nine + [2, 2, big], nine + [2, 3, big - 2],
                       nine + [2, 2, 0, 0], []],
        EVOLVE: [[8, 1, 0], [8, 1, top + 1], [8, 1, 2, 2], [8, 1, 2, 0, illegal], [0], [1025], [8, 0], nine + [0], nine + [257], nine + [4, -1], nine + [4, 65],
                 nine + [4, 1, 0], nine + [4, 1, 5], nine + [4, 1, 1, -1], nine + [4, 1, 1, big], nine + [4, 1, 1, 0, -1], nine + [4, 1, 1, 0, 257],
                 nine + [4, 1, 1, 0, 64, -2], nine + [4, 1, 1, 0, 64, L * L], nine + [4, 1, 1, 0, 64, -1, 0], []],
    }
    # two faults in one row: the message is the first check's
    double = {q: [[0, 0]] for q in single}                                                        # frames + hold
    double[LOOKAHEAD] += [[8, 0, illegal], [8, 1, illegal, illegal]]                              # hold + first, first + rest
    double[ALL] += [[8, 1, illegal, illegal], [8, 0, illegal, illegal]]                           # a bad first, which _ALL ignores, + rest; hold + both
    double[PLAN] += [[8, 0, top + 1], [8, 1, top + 1, -1], [8, 1, 2, L * L, illegal], [8, 1, 2, -1, illegal]]   # hold + depth, depth + code, code + rest
    for q in (SEARCH, SEARCH_SAMPLES):
        double[q] += [[8, 0, 0], [8, 1, 0, 2], [8, 1, too_deep, 2], [8, 1, too_deep, 2, illegal], [8, 1, 2, 2, illegal]]   # .., plan count + objective, objective + rest
    for q in (BEAM, BEAM_SAMPLES, EVOLVE):
        double[q] += [[8, 0, 0], [8, 1, 0, 2], [8, 1, top + 1, 2], [8, 1, 2, 2, illegal]]          # hold + depth, depth + objective, objective + rest
    double[SAMPLES] += [[8, 0, 0], [8, 1, 0, -1], [8, 1, 4097, big], [8, 1, 4, -1, illegal], [8, 1, 4, big - 3, illegal], [8, 1, 0, 0, illegal]]   # samples + salt, salt + rest
    rest_bad = [8, 1, 2, 0, illegal, 0, 0, 0, 0]
    double[SEARCH_SAMPLES] += [rest_bad + [0], nine + [0, -1], nine + [4097, big], [8, 1, too_deep - 1, 0] + tail + [64, big - 2],   # rest + samples, samples + salt,
                               [8, 1, too_deep - 1, 0] + tail + [64, -1], nine + [3, big]]                                             # the leaf cap + salt
    double[BEAM] += [rest_bad + [0], rest_bad + [65]]                                             # rest + width
    double[BEAM_SAMPLES] += [rest_bad + [0], nine + [0, 0], nine + [65, 4097], nine + [2, 0, -1], nine + [2, 4097, big],     # rest + width, width + samples, samples + salt,
                             [8, 1, 5, 0] + tail + [64, cap + 1, big - 2], [8, 1, 5, 0] + tail + [64, cap + 1, -1],          # salt overflow / range + the leaf cap
                             [8, 1, top, 0] + tail + [64, cap + 1, big - 2]]
    double[EVOLVE] += [rest_bad + [0], nine + [0, -1], nine + [257, 65], nine + [4, 65, 0], nine + [4, 1, 0, -1], nine + [4, 1, 5, big],   # rest + population, population +
                       nine + [4, 1, 1, -1, 257], nine + [4, 1, 1, 0, -1, L * L], nine + [4, 1, 1, 0, 257, -3]]                          # generations, .. elite + plan_seed, .. mutation + init
    rows = [(q, args, False) for q in single for args in single[q] + double[q]]
    # through TBX_QUERY_LOOKAHEAD_ACT: the planners' rows with the planner in front (init = -2 is 159's own value, not a fault there)
    for p in PLANNERS:
        rows += [(ACT, [p] + args, False) for args in single[p] + double[p] if not (p == EVOLVE and len(args) == 15 and args[14] == -2)]
    good = {SEARCH: [8, 1, 2, 0] + tail, SEARCH_SAMPLES: nine + [2, 0], BEAM: nine + [2], BEAM_SAMPLES: nine + [2, 2, 0], EVOLVE: nine + [4, 1, 1, 0, 64, -1]}
    for planner in (150, 151, 152, 154, 159, 0, -1, 153.5):
        rows.append((ACT, [planner] + good[BEAM], False))
    for p in PLANNERS:
        assert len(good[p]) == MOST_ARGS[p]
        rows.append((ACT, [p] + good[p] + [0], False))                                           # one column more than the planner takes
        rows.append((ACT, [p] + good[p], True))                                                   # per-env rows
    rows += [(ACT, [], False), (ACT, [EVOLVE] + nine + [0, -1, 0, 0, 0, -2], False), (ACT, [EVOLVE] + [8, 1, top + 1, 0] + tail + [4, 1, 1, 0, 64, -2], False),
             (ACT, [EVOLVE] + nine + [4, 1, 1, 0, 64, -2, 0], False)]                              # init = -2 over a bad population / depth; 17 arguments
    return rows


def ask(engine, query, args, per_env):
    """(code, message) of a refusal, None where the query answers"""
    try:
        engine.reduce(query, np.tile(np.asarray(args, np.float64), (engine.n_envs, 1)) if per_env else args)
    except ToyboxAmdError as err:
        text = str(err)
        assert text.startswith(PREFIX % err.code)
        return err.code, text[len(PREFIX % err.code):]
    return None


def make_engine(lib, game):
    e = Engine(game, ENVS, lib=lib)
    e.seed(1234)
    e.new_game()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libtoybox_amd.so of the commit the fixture is recorded from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "planner_refusals.json"))
    args = ap.parse_args()
    lib = ctypes.CDLL(os.path.abspath(args.lib))
    _abi.bind(lib)
    out, count = {}, 0
    for game in GAMES:
        e = make_engine(lib, game)
        records = []
        for query, row, per_env in refused_rows(game, legal_count(lib, game)):
            got = ask(e, query, row, per_env)
            assert got is not None, "%s query %d %r: not refused" % (game, query, row)
            records.append({"query": query, "args": row, "per_env": per_env, "code": got[0], "message": got[1]})
        e.close()
        out[game] = records
        count += len(records)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:                           # one record per line
        f.write("{\n" + ",\n".join(' "%s": [\n%s\n ]' % (game, ",\n".join("  " + json.dumps(r, sort_keys=True) for r in out[game])) for game in GAMES) + "\n}\n")
    print("%d refusals recorded from %s into %s" % (count, args.lib, args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
