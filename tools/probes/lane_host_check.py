"""The driver of tools/probes/<type>_host_check.py: the kernels' own dynamics code (csrc/<type>_env.hpp) compiled for the CPU with
<type>_host_check.cpp (the four record-lane programs share their reader, replay loop and generator in lane_host_check.hpp, whose Sim
description mirrors what bind() takes here) and run over every fixture of the type, the check of the record's packing, the draw order and the step logic
that needs no GPU.  The host programs check every runtime index themselves, and `--sanitize` builds the stand-alone program with
-fsanitize=address,undefined and runs it directly.  A type's entry point binds build(), write_fixture() and main() to its kind with
bind(), which takes what differs between the types as data.  Not a program of its own."""
import functools
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OPT = ["-O1"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TYPES = {}                                                            # kind -> what bind() was given


def host_compiler():
    """g++ / c++ / clang++ from the PATH, else the clang++ that hipcc itself drives (the build needs ROCm anyway)."""
    for cc in ("g++", "c++", "clang++"):
        if shutil.which(cc):
            return cc
    rocm = os.path.join(os.path.dirname(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "llvm", "bin", "clang++")
    if os.path.exists(rocm):
        return rocm
    raise RuntimeError("no host C++ compiler found (g++, c++, clang++, ROCm's clang++)")


def build(kind, outdir, flags=OPT, compiler=None):
    """the host program of the kind, built into outdir with the given compiler flags; returns its path"""
    exe = os.path.join(outdir, "check")
    subprocess.run([compiler or host_compiler(), *flags, "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "probes", kind + "_host_check.cpp"), "-o", exe],
                   check=True)
    return exe


def write_fixture(kind, name, outdir, edit=None):
    """the fixture as the binary file that the kind's host program reads; returns its path.  edit(arrays) may change the fixture's
    arrays first (tests/test_host_check_detects_cpu.py writes files that the program must refuse)"""
    spec = TYPES[kind]
    with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) as z:
        z = {k: z[k] for k in z.files}
    if edit:
        edit(z)
    n, T = z["reward"].shape
    obs = np.ascontiguousarray(np.bitwise_xor.accumulate(z["obs_xor"], axis=2).transpose(0, 2, 1))      # uint32 [n, T, width]
    reset_at = np.full((n, T), -1, np.int32)
    for j, (i, t) in enumerate(z["reset_index"]):
        reset_at[i, t] = j
    pokes = z.get("pokes", np.zeros((0, 4)))
    names = json.loads(str(z["poke_fields"])) if "poke_fields" in z else []
    header = [n, T, int(z["autoreset"]), len(z["reset_index"])] + [int(z[k]) for k in spec["header"]] + ([len(pokes)] if spec["pokes"] else [])
    path = os.path.join(outdir, name + ".bin")
    with open(path, "wb") as f:
        f.write(np.array(header, np.int32).tobytes())
        f.write(z["reset_obs"].astype(np.float32).tobytes())
        if spec["pokes"]:
            for i, t, k, value in pokes:                              # the named field of env i is set before step t
                f.write(struct.pack("<ii24sd", int(i), int(t), names[int(k)].encode(), float(value)))
        for i in range(n):
            f.write(np.array([int(z["seed0"]) + i], np.int32).tobytes())
            f.write(z["actions"][i].astype(np.int32).tobytes())
            f.write(reset_at[i].tobytes())
            f.write(z["obs0"][i].astype(np.float32).tobytes())
            if spec["info0"]:
                f.write(z["info0"][i].astype(np.float64).tobytes())
            f.write(obs[i].tobytes())
            f.write(z["reward"][i].astype(np.float64).tobytes())
            f.write(z["terminated"][i].astype(np.uint8).tobytes())
            if spec["truncated"]:
                f.write(z["truncated"][i].astype(np.uint8).tobytes())
            f.write(z["info"][i].astype(np.float64).tobytes())
    return path


def main(kind):
    """[--sanitize] and one of the kind's extra modes, which goes to the host program with its arguments, or else every fixture"""
    spec = TYPES[kind]
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(kind, tmp, OPT + (SANITIZE if "--sanitize" in sys.argv else []))
        for mode, nargs in spec["modes"]:
            if mode in sys.argv:
                at = sys.argv.index(mode)
                sys.exit(subprocess.run([exe, *sys.argv[at:at + 1 + nargs]]).returncode)
        for name in spec["fixtures"]:
            subprocess.run([exe, spec["write_fixture"](name, tmp)], check=True)


def bind(kind, fixtures, header=(), pokes=False, info0=False, truncated=False, modes=(), writer=None):
    """-> (build, write_fixture, main) of the kind.  header: the fixture's integers behind the four common ones of the file's header;
    pokes: a poke count and the poke table follow; info0 / truncated: those columns are written; modes: (flag, argument count) of the
    host program's other modes; writer: the type's own write_fixture(name, outdir) where the file is not a record-lane one."""
    writer = writer or functools.partial(write_fixture, kind)
    TYPES[kind] = dict(fixtures=fixtures, header=header, pokes=pokes, info0=info0, truncated=truncated, modes=modes, write_fixture=writer)
    return functools.partial(build, kind), writer, functools.partial(main, kind)
