"""Branch reach of the oracle's game rules (test support, like the *_replay.py modules; nothing here touches a GPU).

The device kernels are held to the oracle bit for bit, but only on the inputs the tests feed: a rule branch no input takes is a place
where a kernel can be wrong with the suite green.  measure() says which branches those are:

* it compiles oracle/*.c with gcc --coverage into a directory of the caller's (objects, .gcno and .gcda all live there: nothing lands
  under oracle/, the ordinary liboracle.so is not touched),
* runs a list of input scripts over that library alone in a fresh child process (the counters are written when it exits) -- a script
  is "module:function", a function of one argument, the loaded library (tests/rule_inputs.py REACH functions, the cases of
  tests/test_gpu_rule_edges.py),
* runs gcov -b (JSON) and returns, per source file and function, the lines never executed and the (line, branch) pairs never taken.

The scope is whole rule files (minus OUT_OF_SCOPE), or a set of functions of any file of the oracle: tests/test_wrapper_reach.py holds the
agent wrapper functions of orc_abi.c that way.

The child runs with TBX_ORACLE_THREADS=1: the counters are plain increments, and a racing pair of increments must not be what decides
between "taken once" and "never"."""
import gzip
import json
import os
import shutil
import subprocess
import sys

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
ORACLE = os.path.join(ROOT, "oracle")
CFLAGS = ["--coverage", "-O1", "-fPIC", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fopenmp"]

# the rule files: step, new game and render of each game with their static helpers (orc_amidar_query and the ABI layer are not rules)
RULE_FILES = {"breakout": "orc_breakout.c", "space_invaders": "orc_si.c", "amidar": "orc_amidar.c", "gridworld": "orc_gridworld.c"}
OUT_OF_SCOPE = {"orc_amidar.c": {"orc_amidar_query"}}


def _gcov_writes_json():
    """gcov -j with a function name per line came with gcc 9 and 10; an older gcov knows no such option"""
    try:
        out = subprocess.run(["gcov", "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True).stdout
        ver = subprocess.run(["gcov", "-dumpversion"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, universal_newlines=True).stdout
    except OSError:
        return False
    major = ver.strip().split(".")[0]
    return "--json-format" in out and (not major.isdigit() or int(major) >= 10)


def missing_tools():
    """the names of the tools measure() needs and this machine lacks"""
    missing = [t for t in ("gcc", "gcov") if shutil.which(t) is None]
    if "gcov" not in missing and not _gcov_writes_json():
        missing.append("a gcov with JSON output (gcc 10 or later)")
    return missing


def build(workdir):
    """oracle/*.c -> workdir/liboracle_reach.so, instrumented; returns its path"""
    srcs = sorted(f for f in os.listdir(ORACLE) if f.startswith("orc_") and f.endswith(".c"))
    objs = []
    for src in srcs:
        obj = os.path.join(workdir, src[:-2] + ".o")
        subprocess.check_call(["gcc"] + CFLAGS + ["-c", os.path.join(ORACLE, src), "-o", obj], cwd=workdir)
        objs.append(obj)
    lib = os.path.join(workdir, "liboracle_reach.so")
    subprocess.check_call(["gcc", "--coverage", "-fopenmp", "-shared", "-Wl,-Bsymbolic", "-o", lib] + objs + ["-lm", "-lrt"], cwd=workdir)
    return lib


def run(lib, scripts, timeout=None):
    """the scripts, in order, over `lib` in one fresh child process; its exit writes the counters beside the objects"""
    env = dict(os.environ, TBX_ORACLE_THREADS="1", OMP_NUM_THREADS="1")
    env["PYTHONPATH"] = os.pathsep.join([TESTS, ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    subprocess.check_call([sys.executable, "-c", "import rule_reach; rule_reach._child()", lib] + list(scripts), env=env, cwd=TESTS, timeout=timeout)


def _child():
    import ctypes
    import importlib
    from toybox_amd import _abi
    lib = ctypes.CDLL(sys.argv[1])
    _abi.bind(lib)
    for script in sys.argv[2:]:
        module, function = script.split(":")
        getattr(importlib.import_module(module), function)(lib)


def in_scope(scope, f, function):
    """scope None: every function of the file but OUT_OF_SCOPE's; else {file: names}: those functions alone.  A name also stands for the
    bodies gcc outlines from it (an OpenMP loop of tbx_agent_reset is reported as tbx_agent_reset._omp_fn.0)"""
    if scope is None:
        return function not in OUT_OF_SCOPE.get(f, set())
    return function.split("._omp_fn.")[0] in scope.get(f, ())


def report(workdir, files, scope=None):
    """gcov -b over the counters in workdir -> {file: {function: {"lines": n, "branches": n, "unexecuted": [line], "untaken": [(line, k)]}}}
    plus, under the key (file, "text"), the file's lines (1-based list index - 1) for allow-lists that go by line text.  scope: in_scope"""
    out = {}
    for f in files:
        stem = f[:-2]
        subprocess.check_call(["gcov", "-b", "-j", "-o", workdir, os.path.join(workdir, stem + ".gcda")], cwd=workdir, stdout=subprocess.DEVNULL)
        with gzip.open(os.path.join(workdir, stem + ".gcov.json.gz"), "rt") as fh:
            js = json.load(fh)
        entry = [x for x in js["files"] if os.path.basename(x["file"]) == f][0]
        funcs = {fn["name"]: {"lines": 0, "branches": 0, "unexecuted": [], "untaken": []} for fn in entry["functions"] if in_scope(scope, f, fn["name"])}
        for ln in entry["lines"]:
            fn = funcs.get(ln.get("function_name"))
            if fn is None:
                continue
            fn["lines"] += 1
            if ln["count"] == 0:
                fn["unexecuted"].append(ln["line_number"])
            for k, br in enumerate(ln["branches"]):
                fn["branches"] += 1
                if br["count"] == 0:
                    fn["untaken"].append((ln["line_number"], k))
        out[f] = funcs
        with open(os.path.join(ORACLE, f)) as fh:
            out[(f, "text")] = fh.read().split("\n")
    return out


def measure(workdir, scripts, games, timeout=None):
    """build, run, report for the rule files of `games`"""
    run(build(workdir), scripts, timeout)
    return report(workdir, [RULE_FILES[g] for g in games])


def table(result):
    """[(file, lines executed, lines, branches taken, branches)] of a report"""
    rows = []
    for f, funcs in result.items():
        if isinstance(f, tuple):
            continue
        nl = sum(v["lines"] for v in funcs.values()); nb = sum(v["branches"] for v in funcs.values())
        rows.append((f, nl - sum(len(v["unexecuted"]) for v in funcs.values()), nl, nb - sum(len(v["untaken"]) for v in funcs.values()), nb))
    return rows


def listing(result):
    """the untaken branches and unexecuted lines as text lines "file:line function [branches k, ..]: source text" """
    rows = []
    for f, funcs in result.items():
        if isinstance(f, tuple):
            continue
        text = result[(f, "text")]
        for name, v in funcs.items():
            by_line = {}
            for line, k in v["untaken"]:
                by_line.setdefault(line, []).append(k)
            for line in sorted(set(by_line) | set(v["unexecuted"])):
                what = "never executed" if line in v["unexecuted"] else "branches %s never taken" % by_line[line]
                rows.append("%s:%d %s, %s: %s" % (f, line, name, what, text[line - 1].strip()))
    return rows


if __name__ == "__main__":
    # python tests/rule_reach.py game[,game] module:function ...   -- prints the table and the listing
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        res = measure(tmp, sys.argv[2:], sys.argv[1].split(","))
    for row in table(res):
        print("%s: lines %d / %d, branches %d / %d" % row)
    print("\n".join(listing(res)))
