"""The yardstick of the act tests (TBX_QUERY_LOOKAHEAD_ACT, include/toybox_amd.h): PLAN ON A CLONE, PICK, STEP, SHIFT, CARRY.

Written from the header's text alone: nothing of the product's plan_pick / plan_shift / act_args is imported.  The planner's rows
come from the replay modules of the planners on the checker (search_replay, search_samples_replay, beam_replay, beam_samples_replay,
evolve_replay); the pick is a sort of tuples of Python integers per env, the carry is Python integer arithmetic, and the closed loop
steps a checker engine with the picked actions and hands the carry on as the next period's per-env init."""
import numpy as np

from beam_replay import expected_beam
from beam_samples_replay import expected_beam_samples
from evolve_replay import expected_evolve
from fork_replay import sim_rngs
from lookahead_replay import FIELDS, MAX_FRAMES
from search_replay import expected_search
from search_samples_replay import SAMPLE_FIELDS, expected_search_samples
from support import LEGAL

SEARCH, SEARCH_SAMPLES, BEAM, BEAM_SAMPLES, EVOLVE, ACT = 153, 155, 156, 157, 158, 159
PLANNERS = (SEARCH, SEARCH_SAMPLES, BEAM, BEAM_SAMPLES, EVOLVE)
SAMPLED = (SEARCH_SAMPLES, BEAM_SAMPLES)
MOST_COLUMNS = {SEARCH: 9, SEARCH_SAMPLES: 11, BEAM: 10, BEAM_SAMPLES: 12, EVOLVE: 15}
BUF_PLAN_ACTION, BUF_PLAN_CARRY = 17, 18
WIDTH = 11
PLAN_MAX_DEPTH = {"breakout": 16, "space_invaders": 12, "amidar": 12, "gridworld": 13}
BATCH_FRAMES = {"breakout": 400, "space_invaders": 400, "amidar": 400, "gridworld": 40}


def planner_rows(lib, game, states, rngs, planner, case):
    """the planner's rows on the checker: a dict of [n, n_legal] arrays, the five fields or the eight sums, and the code.
    case: the keyword arguments of the planner's replay (objective 0 or 1)"""
    if planner == SEARCH:
        return expected_search(lib, game, states, rngs, case)
    if planner == SEARCH_SAMPLES:
        return expected_search_samples(lib, game, states, rngs, case)
    if planner == BEAM:
        return expected_beam(lib, game, states, rngs, case)[0]
    if planner == BEAM_SAMPLES:
        return expected_beam_samples(lib, game, states, rngs, case)[0]
    if planner == EVOLVE:
        return expected_evolve(lib, game, states, rngs, case)[0]
    raise ValueError("no such planner: %r" % (planner,))


def sort_key(rows, planner, objective, i, a):
    """what the pick sorts ascending, a tuple of Python integers: larger-is-better keys negated, the tie-break last"""
    if planner in SAMPLED:
        ret, lost, safe = int(rows["ret_sum"][i, a]), int(rows["lost"][i, a]), int(rows["safe_frames_sum"][i, a])
        return ((-ret, lost, -safe) if objective == 0 else (lost, -safe, -ret)) + (a,)
    at = int(rows["life_lost_at"][i, a])
    ret, lives, loss = int(rows["ret"][i, a]), int(rows["lives"][i, a]), MAX_FRAMES + 1 if at < 0 else at
    return ((-ret, -lives, -loss) if objective == 0 else (-lives, -loss, -ret)) + (int(rows["code"][i, a]),)


def pick(rows, planner, objective):
    """the winner a* of every env, int64 [n]"""
    n, L = np.shape(rows["code"])
    return np.array([min(range(L), key=lambda a: sort_key(rows, planner, objective, i, a)) for i in range(n)], np.int64)


def all_keys_tied(rows, planner, objective):
    """envs in which two or more first actions tie with the winner on every key but the tie-break: bool [n]"""
    n, L = np.shape(rows["code"])
    best = pick(rows, planner, objective)
    return np.array([sum(sort_key(rows, planner, objective, i, a)[:-1] == sort_key(rows, planner, objective, i, int(best[i]))[:-1] for a in range(L)) >= 2
                     for i in range(n)], bool)


def shift(L, code, depth):
    """the carry of a code: the played digit wraps to the end (Python integers)"""
    code = int(code)
    return code // L + (code % L) * L ** (depth - 1)


def out_rows(game, rows, planner, best):
    """out[env][0 .. 10]: the ALE action, the index, the winner's planner row zero-padded to 9"""
    n = len(best)
    names = (SAMPLE_FIELDS if planner in SAMPLED else FIELDS) + ("code",)
    out = np.zeros((n, WIDTH), np.float64)
    for i in range(n):
        a = int(best[i])
        out[i, 0], out[i, 1] = LEGAL[game][a], a
        for c, k in enumerate(names):
            out[i, 2 + c] = float(int(rows[k][i, a]))
    return out


def expected_act(lib, game, states, rngs, planner, case, carry=None):
    """one TBX_QUERY_LOOKAHEAD_ACT on the checker -> (out float64 [n, 11], action int32 [n], carry uint32 [n], rows).  case: the
    planner's replay keywords; init = -2 (planner 158): env e is seeded with carry[e] % L ** depth"""
    n, L = len(states), len(LEGAL[game])
    depth, objective = int(case.get("depth", 1)), int(case.get("objective", 0))
    if planner == EVOLVE and np.ndim(case.get("init", -1)) == 0 and case.get("init", -1) == -2:
        case = dict(case, init=np.array([int(c) % L ** depth for c in (np.zeros(n, np.int64) if carry is None else carry)], np.int64))
    rows = planner_rows(lib, game, states, rngs, planner, case)
    best = pick(rows, planner, objective)
    action = np.array([LEGAL[game][a] for a in best], np.int32)
    new_carry = np.array([shift(L, rows["code"][i, best[i]], depth) for i in range(n)], np.uint32)
    return out_rows(game, rows, planner, best), action, new_carry, rows


def raw_step(hold):
    """the raw form of a period: `hold` frames under the picked actions with auto-reset"""
    def step(e, action):
        for _ in range(hold):
            e.step(action, auto_reset=True)
    return step


def expected_rollout(lib, game, e, planner, k, case, step=None, carry=None):
    """The closed loop on the checker engine `e`, which is stepped: each of k periods plans on a clone of e's records (counter
    t + period), picks, steps e with the picked actions (`step`, default: case's hold frames with auto-reset), shifts, and carries
    into the next period's init where the case asks for -2.  -> list of k dicts: out, action, carry, rows, lives (before the step)"""
    step = raw_step(int(case.get("hold", 1))) if step is None else step
    periods = []
    for period in range(k):
        states, rngs = e.get_states(), sim_rngs(e)
        lives = np.asarray(e.scalars()[1]).copy()
        out, action, carry, rows = expected_act(lib, game, states, rngs, planner, dict(case, t=int(case.get("t", 0)) + period), carry)
        step(e, action)
        periods.append(dict(out=out, action=action, carry=carry, rows=rows, lives=lives))
    return periods


# ---------------------------------------------------------------- the cases of tests/test_gpu_act.py
BIG_SEED = (0xABCDE << 32) | 0x1234567
ROW_ENVS = (1, 65, 257)


def row_case(game, planner):
    """the planner's replay keywords of the rows test: fixed rest for the plain planners, drawn rest under a seed above 32 bits
    and a salted game RNG for the sampled ones"""
    fixed = dict(frames=32, hold=4, rest=LEGAL[game][0])
    drawn = dict(frames=32, hold=4, rest=-1, seed=BIG_SEED, t=2 ** 32 - 3, env_offset=70000, salt=1000)
    return {SEARCH: dict(fixed, depth=2, objective=1), SEARCH_SAMPLES: dict(drawn, depth=2, samples=3, objective=0), BEAM: dict(fixed, depth=6, width=3, objective=0),
            BEAM_SAMPLES: dict(drawn, depth=4, width=2, samples=2, objective=1),
            EVOLVE: dict(fixed, depth=8, population=8, generations=2, elite=2, mutation=64, plan_seed=0x9E3779B9, objective=0)}[planner]


# the closed loop: k periods of `hold` frames; 158 from the carry (P 16, G 2, E 4), 156 at width 3
LOOP_PERIODS = 6
LOOP_ENVS = 65
LOOP_FRAMES = {"breakout": 400, "space_invaders": 400, "amidar": 400, "gridworld": 40}


def loop_case(game, planner, hold=8):
    base = dict(frames=4 * hold, hold=hold, depth=4, objective=0, rest=-1, seed=BIG_SEED, t=11)
    if planner == EVOLVE:
        return dict(base, population=16, generations=2, elite=4, mutation=64, plan_seed=77, init=-2)
    return dict(base, width=3)


def loop_stats(periods, after):
    """what the closed-loop tests assert about their own batch: envs whose lives changed across a period (a life lost, or the last
    one and a reset) and envs whose winner changed its first action between consecutive periods.  after: lives behind the loop"""
    lives = [p["lives"] for p in periods] + [np.asarray(after)]
    lost = np.zeros(len(lives[0]), bool)
    for a, b in zip(lives, lives[1:]):
        lost |= a != b
    changed = np.zeros(len(lives[0]), bool)
    for a, b in zip(periods, periods[1:]):
        changed |= a["action"] != b["action"]
    return int(lost.sum()), int(changed.sum())
