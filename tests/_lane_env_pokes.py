"""Pokes of a fixture's `pokes` table into a device snapshot (used by the GPU tests of the types that have a poked fixture).

A poked fixture was recorded with plain state attributes of the reference's env object set between steps (tests/golden/gen/gen_<type>.py).
The device has no entry point for that, and needs none: snapshot() returns the record as 32-bit columns [word][env] behind a 32-byte
header, so a field is rewritten in the blob and restore() hands it back.  Which word holds which field is not retyped here: layout()
builds tools/probes/<type>_host_check.cpp and reads its `--layout`, which finds every offset through the header's own packer.
"""
import functools
import importlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools", "probes"))
# cge_host.hpp: struct SnapHeader { uint64_t magic; int64_t n; uint32_t tag, extra; uint64_t reserved; }, then the handle's arrays in
# registration order, of which the record is the first (tests/test_farm_cpu.py pins both against the sources)
HEADER_BYTES = 32
SNAP_MAGIC = 0x3350414e53454743
_keep = []


@functools.lru_cache(None)
def layout(kind):
    """{field name: (word offset, "f64" | "u32")} of csrc/<kind>_env.hpp's record"""
    hc = importlib.import_module(kind + "_host_check")
    tmp = tempfile.TemporaryDirectory()
    _keep.append(tmp)
    out = subprocess.run([hc.build(tmp.name), "--layout"], check=True, capture_output=True, text=True).stdout
    table = {name: (int(word), fmt) for name, word, fmt in (line.split() for line in out.splitlines())}
    assert table and all(fmt in ("f64", "u32") for _, fmt in table.values())
    return table


def poke_blob(blob, n, table, env, name, value):
    """rewrite the words of field `name` of env `env` in a snapshot of n envs, in place"""
    word, fmt = table[name]
    assert blob.dtype == np.uint8 and blob.ndim == 1 and 0 <= env < n
    raw = struct.pack("<d", float(value)) if fmt == "f64" else struct.pack("<I", int(value))
    for k in range(len(raw) // 4):
        at = HEADER_BYTES + 4 * ((word + k) * n + env)
        assert at + 4 <= blob.size
        blob[at:at + 4] = np.frombuffer(raw[4 * k:4 * k + 4], np.uint8)


def apply(env, n, kind, pokes):
    """pokes = [(env index, field name, value)]: through snapshot() and restore() of a vector env"""
    blob = env.snapshot()
    table = layout(kind)
    magic, count = struct.unpack("<Qq", blob[:16].tobytes())
    assert magic == SNAP_MAGIC and count == n, "not the snapshot layout this helper addresses"
    assert blob.size >= HEADER_BYTES + 4 * n * (max(w for w, _ in table.values()) + 2)
    for i, name, value in pokes:
        poke_blob(blob, n, layout(kind), i, name, value)
    env.restore(blob)
