"""Branch coverage of the oracles' dynamics under the tests' own action streams (used by test_oracle_branch_coverage.py).

build_copy() copies oracle/ and builds the copy with gcc --coverage; replay() runs tests/_oracle_replay.py on it in a child
process; unreached() runs `gcov -b -c` on the counters and returns the dynamics lines that were never executed or have a branch
outcome never taken, keyed by (file, function, stripped source text): no line number, no branch index, so the key survives another
gcc and edits elsewhere in the file.

    python tests/_oracle_coverage.py WORKDIR [streams] [fixtures] [scenarios]     prints the unreached lines of such a run
"""
import gzip
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENVS = ("snake", "crypto", "traffic", "parking", "climate", "fleet", "manufacturing", "hospital")
ALL = 99             # "outcomes" of a line that was never executed
CFLAGS = "-O0 -g --coverage -fPIC -std=c11 -fno-fast-math -ffp-contract=off"


def is_dynamics(function):
    """env_step, write_obs, the per-env reset and their static helpers: every function of orc_<env>.c but the exported API (orc_*:
    create, info, get_state / set_state, ...), the batch driver (batch_*, and the step_action / hash_step hooks it calls)."""
    return not (function.startswith("orc_") or function.startswith("batch_") or function in ("hash_step", "step_action"))


def build_copy(workdir):
    dst = os.path.join(workdir, "oracle")
    shutil.copytree(os.path.join(ROOT, "oracle"), dst, ignore=shutil.ignore_patterns("*.so", "*.gc*", "__pycache__", "_ref"))
    subprocess.run(["make", "-C", dst, "-B"], check=True, stdout=subprocess.DEVNULL, env=dict(os.environ, CFLAGS=CFLAGS))
    return dst


def replay(workdir, parts=()):
    subprocess.run([sys.executable, os.path.join(HERE, "_oracle_replay.py"), workdir, *parts], check=True, cwd=workdir)


def unreached(workdir):
    """{(file, function, source text): (what, outcomes)} for every dynamics line with what = "never executed" or "branch outcome k of m
    never taken" and outcomes = the number of branch outcomes never taken (ALL for a line never executed)."""
    dst = os.path.join(workdir, "oracle")
    out = {}
    for env in ENVS:
        src = f"orc_{env}.c"
        gcda = f"libcge_oracle.so-orc_{env}.gcda"
        assert os.path.exists(os.path.join(dst, gcda)), f"no counters for {src}: the replay never loaded the coverage build"
        subprocess.run(["gcov", "-b", "-c", "--json-format", gcda], check=True, cwd=dst, stdout=subprocess.DEVNULL)
        with gzip.open(os.path.join(dst, gcda[:-5] + ".gcov.json.gz"), "rt") as f:
            report = json.load(f)
        with open(os.path.join(dst, src)) as f:
            text = f.read().split("\n")
        for unit in report["files"]:
            if os.path.basename(unit["file"]) != src:
                continue
            for ln in unit["lines"]:
                fn = ln.get("function_name")
                if not fn or not is_dynamics(fn):
                    continue
                never = [k for k, b in enumerate(ln["branches"]) if b["count"] == 0]
                if ln["count"] == 0:
                    what = "never executed"
                elif never:
                    what = f"branch outcome {', '.join(map(str, never))} of {len(ln['branches'])} never taken"
                else:
                    continue
                out[(src, fn, text[ln["line_number"] - 1].strip())] = (what, ALL if ln["count"] == 0 else len(never))
    return out


def format_lines(lines):
    return "".join(f"{f} {fn}: {what}\n    {text}\n" for (f, fn, text), (what, _) in sorted(lines.items()))


if __name__ == "__main__":
    work = os.path.abspath(sys.argv[1])
    os.makedirs(work, exist_ok=True)
    build_copy(work)
    replay(work, sys.argv[2:])
    res = unreached(work)
    sys.stdout.write(format_lines(res))
    print(f"{len(res)} lines")
