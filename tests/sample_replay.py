"""The yardstick of the sampled-lookahead tests (TBX_QUERY_LOOKAHEAD_SAMPLES, include/toybox_amd.h): CLONE, SALT AND PLAY, then
plain numpy sums.

Future s of first action a is what tests/lookahead_replay.py already plays: a checker clone of the batch, stepped frame by frame
under the schedule {frames, hold, first = legal[a], rest, seed = sample_seed(seed, s), t, env_offset}.  The salt is put into the
clone's input the way tests/test_gpu_fork.py::test_salt expects a salted fork to come out: bytes 0 .. 15 of a state record are the
two words of the game's `rand`, and each becomes splitmix64(word ^ salt_s), salt_s = salt + s where salt is not 0 (GridWorld has
no game RNG: its records are left alone).  Nothing of the device's way of cutting the samples up appears here: play_samples keeps
every future's five fields, aggregate sums them in whatever order it is told."""
import numpy as np

from lookahead_replay import clone, play, schedule_columns, valid_rows
from support import LEGAL, splitmix64
from toybox_amd.engine import SAMPLE_FIELDS, sample_seed

MAX_SAMPLES = 4096
LEAF_FIELDS = ("ret", "lives", "frames_run", "life_lost_at")


def sample_columns(n, frames, samples=1, hold=1, salt=0, rest=-1, seed=0, t=0, env_offset=0):
    """every column of a sample row as an array [n] (rest None: -1)"""
    s = schedule_columns(n, frames, hold=hold, first=-1, rest=rest, seed=seed, t=t, env_offset=env_offset)
    s["samples"] = np.broadcast_to(np.asarray(samples, np.int64), (n,)).copy()
    s["salt"] = np.broadcast_to(np.asarray(salt, np.int64), (n,)).copy()
    return s


def valid_sample_rows(game, c):
    ok = valid_rows(game, c) & (c["samples"] >= 1) & (c["samples"] <= MAX_SAMPLES) & (c["salt"] >= 0) & (c["salt"] < 2 ** 32)
    return ok & ((c["salt"] == 0) | (c["salt"] + c["samples"] - 1 < 2 ** 32))


def salted(game, states, salt_s):
    """a copy of the state records with the game RNG of env i salted by salt_s[i] (0: as it stands)"""
    rec = np.frombuffer(states, np.uint8).reshape(len(states), -1).copy()
    if game != "gridworld":
        for i in np.flatnonzero(salt_s != 0):
            rec[i, :16] = splitmix64(rec[i, :16].view(np.uint64) ^ np.uint64(salt_s[i])).view(np.uint8)
    return type(states).from_buffer_copy(rec.tobytes())


def play_samples(lib, game, states, rngs, case):
    """case: the keyword arguments of sample_columns.  -> (leaves, active): leaves a dict of ret, lives, frames_run, life_lost_at,
    each int64 [S, n, n_legal] with S the largest sample count of a valid row; active bool [S, n]: future s of env i is played"""
    n, L = len(states), len(LEGAL[game])
    c = sample_columns(n, **case)
    ok = valid_sample_rows(game, c)
    top = int(c["samples"][ok].max()) if ok.any() else 0
    leaves = {k: np.zeros((top, n, L), np.int64) for k in LEAF_FIELDS}
    active = np.zeros((top, n), bool)
    for s in range(top):
        active[s] = ok & (s < c["samples"])
        salt_s = np.where(active[s] & (c["salt"] != 0), c["salt"] + s, 0)
        records = salted(game, states, salt_s)
        sched = {k: c[k].copy() for k in ("frames", "hold", "first", "rest", "seed", "t", "env_offset")}
        sched["seed"] = np.array([sample_seed(int(x), s) for x in c["seed"]], np.uint64)
        sched["frames"][~active[s]] = 0                       # (a row that has no future s: refused by play, never read)
        for a, action in enumerate(LEGAL[game]):
            e = clone(lib, game, records, rngs)
            row = play(e, game, dict(sched, first=np.full(n, action, np.int64)))
            e.close()
            for k in LEAF_FIELDS:
                leaves[k][s, :, a] = np.asarray(row[k]).astype(np.int64)
    return leaves, active


def aggregate(leaves, active, order=None):
    """the eight fields, each int64 [n, n_legal], of the futures added one after the other in `order` (None: 0, 1, 2 ...)"""
    top, n, L = leaves["ret"].shape
    out = {k: np.zeros((n, L), np.int64) for k in SAMPLE_FIELDS}
    first = np.ones((n, L), bool)
    for s in (range(top) if order is None else order):
        on = np.broadcast_to(active[s][:, None], (n, L))
        ret, lost_at = leaves["ret"][s], leaves["life_lost_at"][s]
        out["ret_min"] = np.where(on & (first | (ret < out["ret_min"])), ret, out["ret_min"])
        out["ret_max"] = np.where(on & (first | (ret > out["ret_max"])), ret, out["ret_max"])
        first = first & ~on
        out["samples"] += on
        out["ret_sum"] += np.where(on, ret, 0)
        out["lives_sum"] += np.where(on, leaves["lives"][s], 0)
        out["lost"] += on & (lost_at >= 0)
        out["ended"] += on & (leaves["lives"][s] <= 0)
        out["safe_frames_sum"] += np.where(on, np.where(lost_at < 0, leaves["frames_run"][s], lost_at), 0)
    return out


def expected_samples(lib, game, states, rngs, case):
    """case: frames, samples, hold, salt, rest, seed, t, env_offset (scalars or one per env) -> the eight fields [n, n_legal]"""
    return aggregate(*play_samples(lib, game, states, rngs, case))


def coverage(exp):
    """what the coverage conditions count over the (env, first action) groups of expected rows: groups in all, groups whose
    futures differ in their return, groups where some but not all futures lost a life, groups with an ended future, groups where
    every future lost a life, groups with a return above 0"""
    S = exp["samples"]
    on = S > 0
    return dict(groups=int(on.sum()), spread=int((on & (exp["ret_min"] < exp["ret_max"])).sum()), some_lost=int((on & (exp["lost"] > 0) & (exp["lost"] < S)).sum()),
                ended=int((on & (exp["ended"] > 0)).sum()), all_lost=int((on & (exp["lost"] == S)).sum()), scored=int((on & (exp["ret_max"] > 0)).sum()))


def assert_samples_equal(got, want, what):
    for k in SAMPLE_FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g.astype(np.int64), w.astype(np.int64)):
            bad = np.argwhere(g.astype(np.int64) != w.astype(np.int64))
            i = tuple(bad[0])
            raise AssertionError("%s: %s differs in %d entries, first at %s: got %r, want %r" % (what, k, len(bad), i, g[i], w[i]))


def best_action(rows, objective):
    """the winner among the rows [n, L] of every env, a plain loop.  "return": the largest ret_sum, then the smallest lost, then
    the largest safe_frames_sum, then the smallest index; "survival": the smallest lost, the largest safe_frames_sum, the largest
    ret_sum, the smallest index"""
    n, L = rows["ret_sum"].shape
    best = np.zeros(n, np.int64)
    for i in range(n):
        def key(a):
            r, lo, sf = int(rows["ret_sum"][i, a]), int(rows["lost"][i, a]), int(rows["safe_frames_sum"][i, a])
            return ((-r, lo, -sf) if objective == "return" else (lo, -sf, -r)) + (a,)
        best[i] = min(range(L), key=key)
    return best


# ---------------------------------------------------------------- the cases of tests/test_gpu_samples.py

# (envs, frames, hold, frames of synthetic play behind the batch): tests/lookahead_replay.py batch(); at each of them 8 samples
# replay on the checker in under a second
WORLDS = {"breakout": (24, 160, 4, 400), "space_invaders": (16, 120, 4, 400), "amidar": (24, 96, 4, 400), "gridworld": (24, 24, 2, 40)}
BIG_SEED, BIG_T, ENV_OFFSET = (0xABCDE << 32) | 0x1234567, 2 ** 32 - 3, 70000


def settings(game, frames, hold):
    """name -> case: 1 sample (unchunked), 5 and 33 (uneven chunk bounds), 8; rest fixed and drawn; salt 0 and 1000; a seed above 32
    bits, a counter that crosses 2^32 within the horizon and an env offset.  "coverage" is the case whose figures the GPU module's
    docstring quotes; the 33 samples play a shorter horizon (48 frames: 12 periods) to keep their replay near the others' cost."""
    fixed = LEGAL[game][1]
    assert BIG_T + (min(frames, 48) - 1) // hold >= 2 ** 32
    return {"coverage": dict(frames=frames, hold=hold, samples=8, rest=-1, seed=77),
            "one": dict(frames=frames, hold=hold, samples=1, rest=fixed, seed=5),
            "five": dict(frames=frames, hold=hold, samples=5, salt=1000, rest=-1, seed=BIG_SEED, t=BIG_T, env_offset=ENV_OFFSET),
            "thirtythree": dict(frames=48, hold=hold, samples=33, salt=1000, rest=fixed, seed=BIG_SEED + 1, t=BIG_T, env_offset=ENV_OFFSET),
            "fixed": dict(frames=frames, hold=hold, samples=8, rest=fixed, seed=77),
            "fixed_salted": dict(frames=frames, hold=hold, samples=8, salt=1000, rest=fixed, seed=77),
            "drawn_salted": dict(frames=frames, hold=hold, samples=8, salt=1000, rest=-1, seed=77)}


# the two cases whose difference shows that the salt is read, and whether they must differ: SpaceInvaders fires by its game RNG
# whatever is played; Breakout draws only at a ball start, which fixed actions do not reach; default Amidar and GridWorld draw nothing
SALT_PAIRS = {"space_invaders": ("fixed", "fixed_salted", True), "breakout": ("coverage", "drawn_salted", True),
              "amidar": ("fixed", "fixed_salted", False), "gridworld": ("fixed", "fixed_salted", False)}
