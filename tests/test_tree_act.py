"""Closed-loop tree search (TBX_QUERY_LOOKAHEAD_TREE_ACT, TBX_EDIT_TREE_DROP), the part that needs no GPU: the constants, the
argument shaping, the product's tree_carry and store reader against the replay's own carry (tests/tree_act_replay.py) on random and
hand-built trees, the consequences the header states on the replay itself over the CPU checker, tbx_isqrt on the host, and that the
GPU module's loops cover what they must."""
import functools
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import tree_act_replay as R
from conftest import ROOT
from fork_replay import sim_rngs
from lookahead_replay import batch
from support import LEGAL
from toybox_amd import Engine, ToyboxAmdError, _abi
from toybox_amd.engine import ACT_PLANNERS, TREE_ACT_WIDTH, TREE_FIELDS, plan_pick, tree_act_args, tree_args, tree_carry, tree_store_units
from tree_replay import Node, expected_tree

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
HEADER = open(os.path.join(ROOT, "include", "toybox_amd.h")).read()


def test_header_python_and_replay_agree_on_the_constants():
    want = {"TBX_QUERY_LOOKAHEAD_TREE_ACT": (_abi.QUERY_LOOKAHEAD_TREE_ACT, R.QUERY, 161), "TBX_EDIT_TREE_DROP": (_abi.EDIT_TREE_DROP, R.EDIT_DROP, 44),
            "TBX_BUF_PLAN_TREE": (_abi.BUF_PLAN_TREE, R.BUF_PLAN_TREE, 19), "TBX_BUF_PLAN_ACTION": (_abi.BUF_PLAN_ACTION, R.BUF_PLAN_ACTION, 17),
            "TBX_OPT_TREE_CARRY_KEEP": (_abi.OPT_TREE_CARRY_KEEP, R.OPT_KEEP, 117), "TBX_OPT_TREE_CARRY_MAX_VISITS": (_abi.OPT_TREE_CARRY_MAX_VISITS, R.OPT_MAX_VISITS, 118),
            "TBX_TREE_CARRY_MAX_VISITS": (_abi.TREE_CARRY_MAX_VISITS, R.MAX_VISITS, 4096)}
    for name, (py, replay, value) in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER) or re.search(r"^\s+%s = (\d+),?\s+/\*" % name, HEADER, re.M)     # (the buffer ids: an enum)
        assert m and int(m.group(1)) == py == replay == value, name
    assert re.search(r"#define\s+TBX_QUERY_LOOKAHEAD_TREE_ACT\s+161\s*/\*.*reuse\}\s*->\s*14\s*\*/", HEADER), "columns and width stand on the #define line"
    assert TREE_ACT_WIDTH == R.WIDTH == 14 == 2 + len(TREE_FIELDS) and R.MOST_ARGUMENTS == 13 < _abi.EDIT_MAX_ARGS
    assert _abi.TREE_CARRY_MAX_VISITS == 4 * _abi.TREE_MAX_SIMULATIONS
    text = HEADER[HEADER.index("Closed-loop tree search"):HEADER.index("#define TBX_TREE_CARRY_MAX_VISITS")]
    for consequence in ("(i) ", "(ii) ", "(iii) ", "(iv) ", "(v) ", "(vi) "):
        assert consequence in text, "the header states consequence %s" % consequence
    assert "5120" in text and re.search(r"#define\s+TBX_ABI_VERSION\s+1\b", HEADER)
    assert sorted(ACT_PLANNERS.values()) == [153, 155, 156, 157, 158], "the act planners stay the five"
    declared = set(re.findall(r"\b(tbx_[a-z_0-9]+)\s*\(", HEADER))
    assert declared == set(_abi.PROTOTYPES), "no new symbol: the query, the edit and the store go through what is there"


def test_the_checker_has_no_tree_act(oracle_lib):
    """the expected values cannot come from the checker's own"""
    with Engine("breakout", 4, lib=oracle_lib) as e:
        assert oracle_lib.tbx_reduce_width(_abi.GAME_BREAKOUT, 161) == _abi.E_INVALID
        for call in (lambda: e.reduce(161, [8]), lambda: e.lookahead_tree_act(8, 2, 2), lambda: e.device_buffer(19), lambda: e.tree_drop()):
            with pytest.raises(ToyboxAmdError) as ei:
                call()
            assert ei.value.code == _abi.E_INVALID


# ---------------------------------------------------------------- the argument shaping

def test_tree_act_args_rows():
    assert tree_act_args("breakout", 16, 1) == [16.0, 1.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    seed = (0xDEADBEEF << 32) | 0x12345678
    got = tree_act_args("space_invaders", 300, 12, 1024, 1048576, 2 ** 32 - 1024, True, hold=4, objective="survival", rest=11, seed=seed, t=77, env_offset=4096)
    assert got == [300.0, 4.0, 12.0, 1.0, 11.0, float(0x12345678), float(0xDEADBEEF), 77.0, 4096.0, 1024.0, 1048576.0, float(2 ** 32 - 1024), 1.0]
    assert len(got) == 13 and all(isinstance(v, float) for v in got)
    for game in GAMES:
        kw = dict(frames=24, depth=3, simulations=9, explore=5, salt=2, hold=4, objective=1, rest=LEGAL[game][1], seed=5, t=3, env_offset=9)
        assert tree_act_args(game, reuse=1, **kw)[:12] == list(tree_args(game, 1, **kw)[0]) and tree_act_args(game, reuse=np.bool_(True), **kw)[12] == 1.0


@pytest.mark.parametrize("bad", [dict(frames=0), dict(frames=1025), dict(hold=0), dict(depth=0), dict(depth=17), dict(simulations=0), dict(simulations=1025),
                                 dict(explore=-1), dict(explore=2 ** 20 + 1), dict(salt=-1), dict(salt=2 ** 32), dict(salt=2 ** 32 - 3, simulations=4),
                                 dict(objective=2), dict(objective="score"), dict(rest=2), dict(reuse=2), dict(reuse=-1), dict(reuse="yes"), dict(reuse=np.ones(1)),
                                 dict(depth=np.ones(1)), dict(frames=np.full(1, 8)), dict(simulations=np.ones(1)), dict(explore=np.ones(1)), dict(salt=np.zeros(1)),
                                 dict(seed=2 ** 64), dict(t=2 ** 32), dict(env_offset=-3), dict(n_envs=4)])
def test_tree_act_args_refusals(bad):
    kw = dict(frames=8, depth=2, simulations=4, explore=2)
    kw.update(bad)
    with pytest.raises((ValueError, TypeError)):
        tree_act_args("breakout", **kw)


# ---------------------------------------------------------------- the product's carry against the replay's

def as_nodes(tree, L):
    out = []
    for n, v, child in tree:
        nd = Node(L)
        nd.n, nd.v_sum, nd.child = n, v, [c or None for c in child]
        out.append(nd)
    return out


def as_tuples(nodes):
    return [(nd.n, nd.v_sum, tuple(c or 0 for c in nd.child)) for nd in nodes]


def replay_carry(game, trees, a_star, simulations, keep=0, max_visits=0):
    L = len(LEGAL[game])
    kept, stats = R.carry(as_nodes(trees[a_star], L), L, simulations, keep, max_visits)
    return [as_tuples(t) for t in kept], stats


def random_tree(rng, L, size, depth):
    """a tree in creation order as the search grows it: every new node hangs under an earlier node that lacks that child and is
    above `depth`; visits and values summed up from the leaves"""
    nodes, level = [[0, 0, [0] * L]], [1]
    while len(nodes) < size:
        open_ = [(i, k) for i, nd in enumerate(nodes) if level[i] < depth for k in range(L) if not nd[2][k]]
        if not open_:
            break
        i, k = rng.choice(open_)
        nodes[i][2][k] = len(nodes)
        nodes.append([0, 0, [0] * L])
        level.append(level[i] + 1)
    for i in range(len(nodes) - 1, -1, -1):
        own, value = rng.randint(1, 40), rng.randint(0, 5000)
        nodes[i][0] += own
        nodes[i][1] += value
        for j, nd in enumerate(nodes[:i]):
            if i in nd[2]:
                nd[0] += nodes[i][0]
                nd[1] += nodes[i][1]
    return [(n, v, tuple(c)) for n, v, c in nodes]


@pytest.mark.parametrize("game", GAMES)
def test_tree_carry_is_the_replays_carry_on_random_trees(game):
    rng = random.Random(GAMES.index(game))
    L = len(LEGAL[game])
    seen = dict(truncated=0, halved=0, absent=0)
    for trial in range(60):
        simulations = rng.choice([1, 3, 8, 30])
        trees = [random_tree(rng, L, rng.randint(1, 2 * simulations + 1), rng.choice([1, 2, 3, 5])) for _ in range(L)]
        a_star = rng.randrange(L)
        keep = rng.choice([0, 0, 1, 2, 5, simulations + 1])
        top = [trees[a_star][c][0] for c in trees[a_star][0][2] if c]
        max_visits = rng.choice([0, 1, 4096] + top + [t - 1 for t in top if t > 1])
        want, stats = replay_carry(game, trees, a_star, simulations, min(keep, simulations + 1), max_visits)
        got = tree_carry(game, trees, a_star, simulations, keep=keep or None, max_visits=max_visits or None)
        assert got == want, (game, trial)
        for k in seen:
            seen[k] += stats[k]
        for tree in got:
            assert len(tree) <= min(keep or simulations + 1, simulations + 1) and all(0 <= c < len(tree) and (c == 0 or c > i) for i, nd in enumerate(tree) for c in nd[2])
    assert all(seen.values()), seen


def test_tree_carry_hand_built_cases():
    game, L = "breakout", 4
    # tree a* = 1.  Root 0 has children 1 (digit 0) and 2 (digit 2): digits 1 and 3 are absent.  Subtree of digit 0: ids 1, 3, 4, 6
    # (3 and 4 under 1, 6 under 3); subtree of digit 2: ids 2, 5, 7 (5 under 2, 7 under 5).
    tree = [(20, 900, (1, 0, 2, 0)), (12, 500, (3, 4, 0, 0)), (8, 400, (0, 5, 0, 0)), (7, 300, (0, 0, 6, 0)), (4, 150, (0, 0, 0, 0)), (5, 250, (7, 0, 0, 0)),
            (3, 101, (0, 0, 0, 0)), (2, 99, (0, 0, 0, 0))]
    other = [(1, 5, (0, 0, 0, 0))]
    trees = [other, tree, other, other]
    full = tree_carry(game, trees, 1, 8)
    assert full == [[(12, 500, (1, 2, 0, 0)), (7, 300, (0, 0, 3, 0)), (4, 150, (0, 0, 0, 0)), (3, 101, (0, 0, 0, 0))], [],
                    [(8, 400, (0, 1, 0, 0)), (5, 250, (2, 0, 0, 0)), (2, 99, (0, 0, 0, 0))], []], "two absent children, both subtrees whole"
    # keep = 3: id 6 of the digit-0 subtree falls -- a node in the middle of tree a*, with id 7 of the OTHER subtree, a larger id, kept
    cut = tree_carry(game, trees, 1, 8, keep=3)
    assert cut[0] == [(12, 500, (1, 2, 0, 0)), (7, 300, (0, 0, 0, 0)), (4, 150, (0, 0, 0, 0))] and cut[2] == full[2], "the link to the dropped node is 0, n and v_sum stay"
    # keep = 1: the new roots alone, every link cut
    assert tree_carry(game, trees, 1, 8, keep=1) == [[(12, 500, (0, 0, 0, 0))], [], [(8, 400, (0, 0, 0, 0))], []]
    # the threshold: a root exactly at it stays, one above is halved with every kept node: n = (n + 1) // 2, v_sum = v_sum // 2
    at = tree_carry(game, trees, 1, 8, max_visits=12)
    assert at == full
    above = tree_carry(game, trees, 1, 8, max_visits=11)
    assert above[0] == [(6, 250, (1, 2, 0, 0)), (4, 150, (0, 0, 3, 0)), (2, 75, (0, 0, 0, 0)), (2, 50, (0, 0, 0, 0))] and above[2] == full[2], "8 <= 11: that tree is not halved"
    assert tree_carry(game, trees, 1, 8, max_visits=7)[2] == [(4, 200, (0, 1, 0, 0)), (3, 125, (2, 0, 0, 0)), (1, 49, (0, 0, 0, 0))]
    # depth 1: a root without children carries nothing
    assert tree_carry(game, trees, 0, 8) == [[], [], [], []]
    for args, kw in (((trees, 1, 8), {}), ((trees, 1, 8), dict(keep=3)), ((trees, 1, 8), dict(keep=1)), ((trees, 1, 8), dict(max_visits=11)), ((trees, 1, 8), dict(max_visits=7))):
        assert tree_carry(game, *args, **kw) == replay_carry(game, args[0], 1, 8, kw.get("keep", 0), kw.get("max_visits", 0))[0]
    for bad in (dict(keep=-1), dict(keep=1026), dict(max_visits=4097), dict(max_visits=-1)):
        with pytest.raises(ValueError):
            tree_carry(game, trees, 1, 8, **bad)
    for bad in ((trees[:3], 1, 8), (trees, 4, 8), (trees, 1, 0), (trees, 1, 1025)):
        with pytest.raises(ValueError):
            tree_carry(game, *bad)


def test_the_store_reader_reads_the_documented_layout():
    game, L, simulations = "gridworld", 5, 3
    stride = 4                                                     # (3 + 2) & ~1
    block = 64 + 32 * stride
    raw = np.zeros((2, L, block), np.uint8)
    node = np.dtype([("v_sum", "<i8"), ("n", "<u4"), ("child", "<u2", (6,)), ("zero", "<u8")])
    assert node.itemsize == 32
    raw[1, 3, :4] = np.array([2], "<u4").view(np.uint8)
    recs = np.zeros(stride, node)
    recs[0] = (700, 9, (0, 1, 0, 0, 0, 0), 0)
    recs[1] = (300, 4, (0, 0, 0, 0, 0, 0), 0)
    recs[2] = (-1, 77, (5, 5, 5, 5, 5, 5), 0)                      # past the count: unspecified, never read
    raw[1, 3, 64:] = recs.view(np.uint8)
    units = tree_store_units(game, raw.reshape(-1), 2, simulations)
    assert units[1][3] == [(9, 700, (0, 1, 0, 0, 0)), (4, 300, (0, 0, 0, 0, 0))]
    assert all(units[e][k] == [] for e in range(2) for k in range(L) if (e, k) != (1, 3))


# ---------------------------------------------------------------- tbx_isqrt on the host

def test_isqrt_is_exact_on_the_host(tmp_path):
    """tbx_isqrt is __host__ __device__: a stand-alone host program (tests/tree_isqrt_check.hip) compares it with an integer root
    for every n << 16, n in 0 .. 5120, and around every square in and far beyond that range"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "isqrt_check")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-host-only", "-w", "-o", exe, os.path.join(ROOT, "tests", "tree_isqrt_check.hip")], check=True)
    done = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(done.stdout)
    assert done.returncode == 0 and re.search(r"checked (\d+) bad 0", done.stdout) and int(re.search(r"checked (\d+)", done.stdout).group(1)) > 5120


# ---------------------------------------------------------------- the consequences, on the replay alone

N = 8


@pytest.fixture(scope="module")
def batches(oracle_lib):
    out = {}
    for game in GAMES:
        e = batch(oracle_lib, game, N)
        out[game] = (e.get_states(), sim_rngs(e))
        e.close()
    return out


@pytest.mark.parametrize("game", GAMES)
def test_the_consequences_hold_for_the_replay(game, batches, oracle_lib):
    states, rngs = batches[game]
    L, hold = len(LEGAL[game]), R.HOLD[game]
    tree = dict(frames=hold * 6, hold=hold, depth=3, objective=0, simulations=3 * L + 1, explore=7, rest=-1, seed=(5 << 33) | 3, t=9, env_offset=11, salt=5)
    # (i) reuse = 0: the row of a* is query 160's, and a* the sampled planners' pick on 160's rows (the product's plan_pick)
    plain, _, _ = expected_tree(oracle_lib, game, states, rngs, tree)
    st = R.TreeActReplay(game, N)
    first = st.call(oracle_lib, states, rngs, tree, 0)
    rows160 = np.stack([plain[k] for k in TREE_FIELDS[:8]] + [plain["code"]], axis=2)
    assert np.array_equal(first["best"], plan_pick(rows160, 0, sampled=True))
    for i in range(N):
        a = int(first["best"][i])
        assert first["out"][i].tolist() == [float(LEGAL[game][a]), float(a)] + [float(plain[k][i, a]) for k in TREE_FIELDS]
    # (iii) samples = M in every row, with and without carried trees
    assert (first["rows"]["samples"] == tree["simulations"]).all()
    # (ii) reuse = 1 without a live tree equals reuse = 0: the first call, a changed key, dropped envs
    fresh = R.TreeActReplay(game, N).call(oracle_lib, states, rngs, tree, 1)
    assert np.array_equal(fresh["out"], first["out"]) and fresh["stats"]["used"] == 0
    other_key = st.call(oracle_lib, states, rngs, dict(tree, depth=2), 1)
    assert other_key["stats"]["used"] == 0 and np.array_equal(other_key["out"], R.TreeActReplay(game, N).call(oracle_lib, states, rngs, dict(tree, depth=2), 0)["out"])
    st.call(oracle_lib, states, rngs, tree, 0)
    assert st.drop(None) and st.flags.all()
    dropped = st.call(oracle_lib, states, rngs, tree, 1)
    assert dropped["stats"]["used"] == 0 and dropped["stats"]["flag_drops"] == N and np.array_equal(dropped["out"], first["out"]) and not st.flags.any()
    # a live tree is used, its statistics steer and are not counted: samples stays M while the roots have seen more than M
    again = st.call(oracle_lib, states, rngs, tree, 1)
    assert again["stats"]["used"] > 0 and (again["rows"]["samples"] == tree["simulations"]).all()
    assert max(t[0].n for env in again["trees"] for t in env) > tree["simulations"] and all(t[0].n >= tree["simulations"] for env in again["trees"] for t in env)
    # the store is the product's carry of the final trees (v): the same function, two implementations
    for i in range(N):
        a = int(again["best"][i])
        final = [as_tuples(t) for t in again["trees"][i]]
        assert st.units()[i] == tree_carry(game, final, a, tree["simulations"]), (game, i)
    assert not R.TreeActReplay(game, N).drop(None), "the edit is refused before the first call"


# ---------------------------------------------------------------- the GPU module's loops cover what they must

@functools.lru_cache(maxsize=None)
def loop_replay(oracle_lib, game, name):
    e = batch(oracle_lib, game, R.ENVS, frames=R.BATCH_FRAMES[game])
    kw = R.loop_tree(game, name)
    out, _ = R.expected_loop(oracle_lib, game, e, R.PERIODS, compare=name in ("reuse", "long"), drops={2: R.DROP_MASK} if name in ("reuse", "reuse_explore") else None, **kw)
    e.close()
    return out


@pytest.mark.parametrize("game", GAMES)
def test_the_loops_cover_what_they_must(game, oracle_lib):
    """over a game's loops (tests/tree_act_replay.py, loop_tree), on the replay alone: the eight coverage conditions"""
    totals = {}
    for name in ("reuse", "long", "few", "keep2", "halve1"):
        for r in loop_replay(oracle_lib, game, name):
            for k, v in list(r["stats"].items()) + [("played", r.get("played", 0)), ("picked", r.get("picked", 0))]:
                totals[k] = totals.get(k, 0) + int(v)
    print(game, totals)
    missing = R.missing_coverage(game, totals)
    assert not missing, "%s: the loops together never show: %s" % (game, ", ".join(missing))


@pytest.mark.parametrize("game", GAMES)
def test_the_forced_loops_force(game, oracle_lib):
    """keep 1 / 2 / 5 truncate in every period -- at depth 3 a subtree under a root's child has at most 1 + L nodes, so keep 5 cuts
    nothing in Breakout (L = 4) and is the "fits exactly" case there; max_visits 1 halves in every period, and HALVE_MID is first
    crossed in the third"""
    L = len(LEGAL[game])
    for name in ("keep1", "keep2", "keep5"):
        cuts = [r["stats"]["truncated"] for r in loop_replay(oracle_lib, game, name)]
        assert all(c > 0 for c in cuts) if 1 + L > int(name[4:]) else not any(cuts), (name, cuts)
    assert all(r["stats"]["halved"] > 0 for r in loop_replay(oracle_lib, game, "halve1"))
    mid = [r["stats"]["halved"] for r in loop_replay(oracle_lib, game, "halve_mid")]
    assert mid[0] == 0 and mid[1] == 0 and mid[2] > 0, mid
    assert all(r["stats"]["used"] == 0 for r in loop_replay(oracle_lib, game, "plain"))
