"""The ratchet over the game rules: every branch of the oracle's step, new-game and render code is taken, and every line executed, by
the inputs the device is compared on -- the shared step-parity scripts (tests/rule_inputs.py) plus the hand-built cases of
tests/test_gpu_rule_edges.py -- except an allow-list written here.  A new rule line that no input reaches fails this test; so does an
allow-list entry that no longer names an untaken branch.

Held: all four games (oracle/orc_breakout.c, orc_si.c, orc_amidar.c, orc_gridworld.c).

The measurement (tests/rule_reach.py) builds an instrumented copy of the oracle in a temporary directory and plays the scripts over it
in a child process with TBX_ORACLE_THREADS=1.  No GPU is involved."""
import pytest

import rule_reach

GAMES = ["breakout", "space_invaders", "amidar", "gridworld"]
SCRIPTS = ["rule_inputs:reach_breakout", "rule_inputs:reach_space_invaders", "rule_inputs:reach_amidar", "rule_inputs:reach_gridworld",
           "test_gpu_rule_edges:reach"]

# (file, function, the line's text, how many of the line's branches are excused, why no state or config that tbx_set_state /
# tbx_set_config accept can take them)
# The two enemy_decide entries hold in the source too (dir is -1 on every path that has not yet chosen, and 0..3 out of opts[]), but
# that gcov reports their other branch as a branch at all comes from how gcc -O1 lays the function out (it threads the paths that
# have chosen past the test): another gcc or optimisation level may report no such branch, and test_the_allow_list_is_live then calls
# the entry stale -- drop it then; the rules have not changed.  "if (dir >= 0) a->dir = dir;" stands twice in enemy_decide
# (EnemyTargetPlayer's copy has both branches taken); the entry's count of 1 is what keeps it from excusing that copy.
ALLOW = [
    ("orc_breakout.c", "start_ball", "if (k >= TBX_BRK_MAX_BALLS) return;", 1,
     "both callers come with n_balls == 0: new_game has just zeroed the record, the step calls it only when no ball is left"),
    ("orc_breakout.c", "put", "if (x < 0 || y < 0 || x >= TBX_BRK_W || y >= TBX_BRK_H) return;", 2,
     "rect() clips to the frame before it calls, digit() is called with constant positions inside it: a negative x or y never arrives"),
    ("orc_si.c", "orc_si_step", "for (int b = 0; b < 64; b++)", 1,
     "the loop picks the k-th set bit of colmask with k drawn below popcount(colmask): it always leaves through its break, never at b == 64"),
    ("orc_amidar.c", "put", "if (x < 0 || y < 0 || x >= TBX_AMI_W || y >= TBX_AMI_H) return;", 2,
     "rect() clips to the frame before it calls, digit() is called with constant positions inside it: a negative x or y never arrives"),
    ("orc_amidar.c", "first_open", "return avoid >= 0 && can_go(s, tx, ty, avoid) ? avoid : -1;", 1,
     "the only caller passes opposite(a->dir) of a dir it has just masked to 0..3: avoid is never negative"),
    ("orc_amidar.c", "enemy_decide", "if (dir < 0) dir = can_go(s, tx, ty, a->dir) ? a->dir : first_open(s, tx, ty, opposite(a->dir));", 1,
     "the two sight arms assign a direction 0..3 and the compiled code sends them past this test: what still reaches it is dir == -1, in every state"),
    ("orc_amidar.c", "enemy_decide", "if (dir >= 0) a->dir = dir;", 1,
     "EnemyRandomMvmt's copy of the line: the dead end's -1 is sent past the test by the compiled code, the rest comes from opts[], which holds 0..3"),
    ("orc_gridworld.c", "orc_gridworld_default_config", "while (id < 4 && keys[id] != rows[y][x]) id++;", 1,
     "no state or config is read here: every character of the constant default board is one of the four keys"),
    ("orc_gridworld.c", "orc_gridworld_step", "if (nx < 0 || ny < 0 || nx >= s->width || ny >= s->height || nx >= TBX_GW_MAX_DIM || ny >= TBX_GW_MAX_DIM) return;", 1,
     "tbx_set_state and tbx_set_config refuse a width or height above TBX_GW_MAX_DIM: the tests against it come after the same tests against width and height"),
    ("orc_gridworld.c", "orc_gridworld_step", "if (id >= s->n_tiles || id >= TBX_GW_MAX_TILES) return;          /* a cell without a tile is a wall */", 1,
     "n_tiles above TBX_GW_MAX_TILES is refused: an id below n_tiles is below the table's size"),
    ("orc_gridworld.c", "orc_gridworld_render", "if (id < s->n_tiles && id < TBX_GW_MAX_TILES) col = s->tiles[id].color;", 1,
     "n_tiles above TBX_GW_MAX_TILES is refused: an id below n_tiles is below the table's size"),
]


def idle(oracle_lib):
    """a script that reaches next to nothing: one new game, one frame of one env"""
    from toybox_amd import Engine
    for game in GAMES:
        with Engine(game, 1, lib=oracle_lib) as e:
            e.new_game()
            e.step([0])


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    missing = rule_reach.missing_tools()
    if missing:
        pytest.skip("the branch-reach measurement needs %s on the PATH" % " and ".join(missing))
    work = str(tmp_path_factory.mktemp("rule_reach"))
    files = [rule_reach.RULE_FILES[g] for g in GAMES]
    lib = rule_reach.build(work)
    rule_reach.run(lib, ["test_rule_reach:idle"])
    dull = rule_reach.report(work, files)
    rule_reach.run(lib, SCRIPTS)                         # (the counters of the two runs add up)
    return dull, rule_reach.report(work, files)


def _allowed(result, f, function, line):
    """how many untaken branches the allow-list excuses on this line (0: none)"""
    text = result[(f, "text")][line - 1].strip()
    return sum(a[3] for a in ALLOW if a[0] == f and a[1] == function and a[2] == text)


def test_every_rule_branch_is_reached(reports):
    _, full = reports
    left = []
    for f in (rule_reach.RULE_FILES[g] for g in GAMES):
        for function, v in full[f].items():
            assert v["lines"] > 0, (f, function)
            left += ["%s:%d %s: line never executed" % (f, line, function) for line in v["unexecuted"] if not _allowed(full, f, function, line)]
            per_line = {}
            for line, k in v["untaken"]:
                per_line.setdefault(line, []).append(k)
            left += ["%s:%d %s: branches %s never taken (%d excused)" % (f, line, function, ks, _allowed(full, f, function, line))
                     for line, ks in sorted(per_line.items()) if len(ks) > _allowed(full, f, function, line)]
    assert not left, "rule code no step-parity input reaches (add a case to tests/test_gpu_rule_edges.py):\n" + "\n".join(left + rule_reach.listing(full))


def test_the_allow_list_is_live(reports):
    """every entry names a line of its function that still has an untaken branch: an entry for code that is gone, or that an input now
    reaches, has to go"""
    _, full = reports
    for f, function, text, count, reason in ALLOW:
        assert reason
        v = full[f][function]
        lines = {line for line, _ in v["untaken"]} | set(v["unexecuted"])
        assert any(full[(f, "text")][line - 1].strip() == text for line in lines), "stale allow-list entry: %s %s: %s" % (f, function, text)
        untaken = [line for line, _ in v["untaken"] if full[(f, "text")][line - 1].strip() == text]
        assert len(untaken) == count, "allow-list entry excuses %d branches, %d are untaken: %s %s: %s" % (count, len(untaken), f, function, text)


def test_the_measurement_sees_what_is_not_reached(reports):
    """the same build under a script that plays one frame: the step's brick, paddle and wall branches are reported untaken there, so an
    empty report above is a finding and not a blind tool"""
    dull, full = reports
    step = dull["orc_breakout.c"]["orc_breakout_step"]
    assert len(step["untaken"]) > 20 and len(step["unexecuted"]) > 10, (len(step["untaken"]), len(step["unexecuted"]))
    assert dull["orc_breakout.c"]["orc_breakout_render"]["unexecuted"], "nothing was rendered in the idle run"
    assert len(dull["orc_si.c"]["orc_si_step"]["unexecuted"]) > 10
    assert len(dull["orc_amidar.c"]["enemy_decide"]["unexecuted"]) > 10 and len(dull["orc_gridworld.c"]["orc_gridworld_step"]["untaken"]) > 3
    for f, function in (("orc_breakout.c", "orc_breakout_step"), ("orc_si.c", "orc_si_step"), ("orc_amidar.c", "enemy_decide"), ("orc_gridworld.c", "orc_gridworld_step")):
        assert not full[f][function]["unexecuted"], (f, function)
