#!/usr/bin/env python3
"""Does evolution find better plans than the beam?  Reported from the CPU replay alone (tests/evolve_replay.py, tests/beam_replay.py
over the checker): no GPU, nothing gated.

On the worlds of the beam tests' deep cases (tests/beam_replay.py, BEAM_CASES[game][0]) and at an equal number of plan plays per
first action -- the beam plays 1 + sum over levels of kept x n_legal candidates; the evolution population + generations x
(population - elite) with elite = population // 4, the (population, generations) with the most plays not above the beam's -- the share
of (env, first action) groups where the evolution's row is better than, equal to, or worse than the beam's under the objective's
keys, cold and warm-started from the beam's own code (then the evolution also spends the beam's plays: the row says what it adds).

    python scripts/evolve_quality.py          # prints a markdown table for profiles/evolve.md
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from beam_replay import BEAM_CASES, case_beam, expected_beam  # noqa: E402
from evolve_replay import expected_evolve, not_worse  # noqa: E402
from fork_replay import sim_rngs  # noqa: E402
from lookahead_replay import batch  # noqa: E402
from support import LEGAL  # noqa: E402
from toybox_amd import _abi  # noqa: E402
from toybox_amd.engine import beam_kept  # noqa: E402

GAMES = ("breakout", "space_invaders", "amidar", "gridworld")


def budget(plays):
    """(population, generations, elite) with elite = population // 4 and 3 .. 8 generations: the most plays not above `plays`"""
    best = None
    for G in range(3, 9):
        for P in range(4, 257):
            E = max(1, P // 4)
            spent = P + G * (P - E)
            if spent <= plays and (best is None or spent > best[0]):
                best = (spent, P, G, E)
    return best


def main():
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    _abi.bind(lib)
    print("| game | shape (envs, frames, hold, depth) | beam width, plays | evolve P, G, E, plays | objective | cold: better / equal / worse | warm: better / equal / worse |")
    print("|---|---|---|---|---|---|---|")
    for game in GAMES:
        case = BEAM_CASES[game][0]
        n, frames, hold, depth, width, batch_frames = case
        L = len(LEGAL[game])
        e = batch(lib, game, n, frames=batch_frames)
        states, rngs = e.get_states(), sim_rngs(e)
        e.close()
        plays = 1 + sum(beam_kept(L, width, d - 1) * L for d in range(2, depth + 1))
        spent, P, G, E = budget(plays)
        for o, objective in enumerate(("return", "survival")):
            beam, _ = expected_beam(lib, game, states, rngs, dict(case_beam(game, case), objective=o))
            ev = dict(frames=frames, hold=hold, depth=depth, objective=o, rest=LEGAL[game][0], population=P, generations=G, elite=E,
                      mutation=max(1, round(256 / max(depth - 1, 1))), plan_seed=1)
            shares = []
            for init in (None, beam["code"]):
                if init is None:
                    rows, _ = expected_evolve(lib, game, states, rngs, ev)
                else:                                        # one init per (env, first action): the beam's code of that group
                    rows = {k: np.zeros_like(v) for k, v in beam.items()}
                    for a in range(L):
                        part, _ = expected_evolve(lib, game, states, rngs, dict(ev, init=init[:, a]))
                        for k in rows:
                            rows[k][:, a] = part[k][:, a]
                ge, le = not_worse(o, rows, beam), not_worse(o, beam, rows)
                shares.append("%.0f%% / %.0f%% / %.0f%%" % (100 * (ge & ~le).mean(), 100 * (ge & le).mean(), 100 * (le & ~ge).mean()))
            print("| %s | (%d, %d, %d, %d) | %d, %d | %d, %d, %d, %d | %s | %s | %s |" % (game, n, frames, hold, depth, width, plays, P, G, E, spent, objective, *shares), flush=True)


if __name__ == "__main__":
    main()
