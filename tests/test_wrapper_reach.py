"""The ratchet over the agent wrapper stack: every line of the oracle's wrapper functions (oracle/orc_abi.c, raw_scalars .. commit_obs and
the per-env loops of tbx_agent_reset and tbx_agent_step_device) and of both functions of oracle/orc_preproc.c is executed, and every
branch taken, by the oracle's side of the cases of tests/test_gpu_wrapper_events.py -- the inputs the device is compared on -- except an
allow-list written here.  A new wrapper line that no case reaches fails this test; so does an allow-list entry that no longer names an
untaken branch.

The measurement is tests/rule_reach.py's, with a set of functions as its scope.  No GPU is involved."""
import pytest

import rule_reach

SCOPE = {"orc_abi.c": {"raw_scalars", "raw_lives", "raw_frame", "base_step", "base_reset", "noop_reset", "skip_step", "monitor_step", "monitor_reset",
                       "episodic_step", "episodic_reset", "top_reset", "commit_obs", "tbx_agent_reset", "tbx_agent_step_device"},
         "orc_preproc.c": {"orc_warp_area", "orc_stack_push"}}
FILES = sorted(SCOPE)
SCRIPTS = ["test_gpu_wrapper_events:reach"]

CONTRACT = "the scope is the call's per-env loop; its argument checks belong to tests/test_gpu_agent_scale.py::test_agent_step_device_call_contract and tests/test_buffer_contract.py"
# (file, function, the line's text, how many of the line's branches are excused, why)
ALLOW = [
    ("orc_abi.c", "tbx_agent_reset", "if (!e) return TBX_E_INVALID;", 1, CONTRACT),
    ("orc_abi.c", "tbx_agent_reset", 'if (!e->agent_on) return fail(e, TBX_E_INVALID, "tbx_agent_init has not been called");', 1, CONTRACT),
    ("orc_abi.c", "tbx_agent_reset", "if (obs && !e->aobs) return agent_no_stack(e);", 1, CONTRACT),
    ("orc_abi.c", "tbx_agent_step_device", "if (!e) return TBX_E_INVALID;", 1, CONTRACT),
    ("orc_abi.c", "tbx_agent_step_device", 'if (!e->agent_on) return fail(e, TBX_E_INVALID, "tbx_agent_init has not been called");', 1, CONTRACT),
    ("orc_abi.c", "tbx_agent_step_device", 'if (!actions) return fail(e, TBX_E_INVALID, "actions pointer is NULL");', 1, CONTRACT),
]


def idle(oracle_lib):
    """a script that reaches next to nothing of the stack: one reset and one step of one GridWorld env with every wrapper off"""
    from toybox_amd import Engine
    with Engine("gridworld", 1, lib=oracle_lib) as e:
        e.agent_init(skip=4, clip_reward=False)
        e.agent_reset()
        e.agent_step([0])


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    missing = rule_reach.missing_tools()
    if missing:
        pytest.skip("the branch-reach measurement needs %s on the PATH" % " and ".join(missing))
    work = str(tmp_path_factory.mktemp("wrapper_reach"))
    lib = rule_reach.build(work)
    rule_reach.run(lib, ["test_wrapper_reach:idle"])
    dull = rule_reach.report(work, FILES, SCOPE)
    rule_reach.run(lib, SCRIPTS)                         # (the counters of the two runs add up)
    return dull, rule_reach.report(work, FILES, SCOPE)


def _allowed(result, f, function, line):
    text = result[(f, "text")][line - 1].strip()
    return sum(a[3] for a in ALLOW if a[0] == f and a[1] == function and a[2] == text)


def test_every_wrapper_branch_is_reached(reports):
    _, full = reports
    left = []
    for f in FILES:
        assert {name.split("._omp_fn.")[0] for name in full[f]} == SCOPE[f], (f, sorted(full[f]))
        for function, v in full[f].items():
            assert v["lines"] > 0, (f, function)
            left += ["%s:%d %s: line never executed" % (f, line, function) for line in v["unexecuted"] if not _allowed(full, f, function, line)]
            per_line = {}
            for line, k in v["untaken"]:
                per_line.setdefault(line, []).append(k)
            left += ["%s:%d %s: branches %s never taken (%d excused)" % (f, line, function, ks, _allowed(full, f, function, line))
                     for line, ks in sorted(per_line.items()) if len(ks) > _allowed(full, f, function, line)]
    assert not left, "wrapper code no case of tests/test_gpu_wrapper_events.py reaches:\n" + "\n".join(left + rule_reach.listing(full))


def test_the_allow_list_is_live(reports):
    """every entry names a line of its function that still has exactly that many untaken branches"""
    _, full = reports
    for f, function, text, count, reason in ALLOW:
        assert reason
        v = full[f][function]
        untaken = [line for line, _ in v["untaken"] if full[(f, "text")][line - 1].strip() == text]
        assert untaken, "stale allow-list entry: %s %s: %s" % (f, function, text)
        assert len(untaken) == count, "allow-list entry excuses %d branches, %d are untaken: %s %s: %s" % (count, len(untaken), f, function, text)


def test_the_measurement_sees_what_is_not_reached(reports):
    """the same build under one plain step: the reset procedure's branches are reported untaken there, so an empty report above is a
    finding and not a blind tool"""
    dull, full = reports
    for function in ("noop_reset", "episodic_step", "episodic_reset", "top_reset", "commit_obs", "skip_step"):
        assert dull["orc_abi.c"][function]["untaken"], function
    assert dull["orc_abi.c"]["top_reset"]["unexecuted"] and dull["orc_abi.c"]["episodic_reset"]["unexecuted"]
    for function in ("noop_reset", "episodic_step", "episodic_reset", "top_reset", "commit_obs", "skip_step"):
        assert not full["orc_abi.c"][function]["untaken"] and not full["orc_abi.c"][function]["unexecuted"], function
