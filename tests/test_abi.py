"""CPU-side checks of the drop-in boundary: libcge_amd.so builds, loads and exports exactly the
entry points include/cge_amd.h declares (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, "include", "cge_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cge_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_full_per_env_surface():
    names = _declared()
    for env in ["snake", "crypto", "traffic"]:
        for fn in ["create", "destroy", "seed", "reset", "step", "rollout", "info", "state_bytes", "get_state",
                   "set_state", "last_error", "device_bytes"]:
            assert f"cge_{env}_{fn}" in names, (env, fn)
    assert "cge_snake_error_count" in names
    for fn in ["create", "destroy", "seed", "reset", "step", "rollout", "info", "info64", "last_error", "device_bytes"]:
        assert f"cge_parking_{fn}" in names, fn
    for env in ["climate", "fleet", "manufacturing", "hospital"]:
        for fn in ["create", "destroy", "seed", "reset", "step", "rollout", "info", "last_error", "device_bytes"]:
            assert f"cge_{env}_{fn}" in names, (env, fn)
    for env in ["parking", "climate", "fleet", "manufacturing", "hospital"]:      # whole-handle checkpoint / resume
        for fn in ["snapshot_bytes", "snapshot_get", "snapshot_set"]:
            assert f"cge_{env}_{fn}" in names, (env, fn)


def test_library_exports_every_declared_symbol():
    from custom_gymnasium_environments_amd import _native, build
    build.build_native()
    L = ctypes.CDLL(_native.LIB_PATH)
    missing = [n for n in _declared() if not hasattr(L, n)]
    assert not missing, missing
    # and the python binding table covers exactly the header
    assert sorted(_native.SIGNATURES) == _declared()


_RESTYPE = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p, "int64_t": ctypes.c_int64,
            "uint32_t": ctypes.c_uint32, "void": None}
_SCALAR = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64}


def test_binding_table_matches_the_header_prototypes():
    """Every prototype of include/cge_amd.h against _native.SIGNATURES: the return type, the number of parameters and each
    parameter's kind (a pointer is c_void_p or a ctypes POINTER, a scalar is the ctypes integer of its width).  A wrong arity
    in the table is otherwise invisible until a GPU call misbehaves."""
    from custom_gymnasium_environments_amd import _native
    src = open(os.path.join(ROOT, "include", "cge_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = re.findall(r"^\s*(const char \*|int64_t|uint32_t|size_t|void|int)\s*(cge_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert sorted(name for _, name, _ in protos) == _declared() == sorted(_native.SIGNATURES)
    for ret, name, args in protos:
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is _RESTYPE[ret], (name, ret, restype)
        params = [] if args.strip() in ("", "void") else [" ".join(p.split()) for p in args.split(",")]
        assert len(argtypes) == len(params), (name, params, argtypes)
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, p, t)
            else:
                assert t is _SCALAR[p.rsplit(" ", 1)[0]], (name, p, t)


def test_host_only_entry_points_work_without_a_gpu(oracle):
    from custom_gymnasium_environments_amd import _native
    L = _native.lib()
    assert b"gfx950" in L.cge_version()
    for args in [(123, 0, 0, 4, 0), (123, 1048575, 999, 4, 0), (7, 77, 12345, 3, 8), (2**63, 5, 6, 5, 0)]:
        assert L.cge_hash_action(*args) == oracle.hash_action(*args)


def _valid_configs(N):
    crypto, traffic = N.CryptoConfig(), N.TrafficConfig()
    L = ctypes.CDLL(N.LIB_PATH)
    L.cge_crypto_default_config(ctypes.byref(crypto))
    L.cge_traffic_default_config(ctypes.byref(traffic))
    return {"snake": N.SnakeConfig(grid_size=10), "crypto": crypto, "traffic": traffic, "parking": N.ParkingConfig(),
            "climate": N.ClimateConfig(max_occupancy=8, episode_minutes=1440), "fleet": N.FleetConfig(),
            "manufacturing": N.ManufacturingConfig(), "hospital": N.HospitalConfig(), "bus": N.BusConfig()}


@pytest.mark.parametrize("env", ["snake", "crypto", "traffic", "parking", "climate", "fleet", "manufacturing", "hospital", "bus"])
def test_create_and_null_handle_answers(env):
    """The entry points every env type shares, through raw ctypes: create's argument / config / device checks in that order (the
    order decides the status code), and what the one-liners answer for a NULL handle."""
    import torch
    from custom_gymnasium_environments_amd import _native as N, build
    build.build_native()
    L = ctypes.CDLL(N.LIB_PATH)
    fn = lambda name, restype=ctypes.c_int: _bind(L, f"cge_{env}_{name}", restype)
    cfg = _valid_configs(N)[env]
    create = fn("create")

    def run(cfg_ptr, n_envs):
        out = ctypes.c_void_p(0xdead)           # a failing create must leave NULL behind
        st = create(cfg_ptr, ctypes.c_int64(n_envs), 0, ctypes.c_int64(0), ctypes.byref(out))
        return st, out.value

    assert run(ctypes.byref(cfg), 0)[0] == -1
    assert run(None, 4)[0] == -1
    mode = cfg.autoreset_mode
    cfg.autoreset_mode = 7
    assert run(ctypes.byref(cfg), 4) == (-1, None)
    cfg.autoreset_mode = mode
    if not torch.cuda.is_available():
        assert run(ctypes.byref(cfg), 4) == (-4, None)
    assert fn("destroy")(None) == -1
    assert fn("device_bytes", ctypes.c_size_t)(None) == 0
    assert fn("last_error", ctypes.c_char_p)(None) == b"null handle"
    assert fn("last_kernel", ctypes.c_char_p)(None) == b""
    assert fn("episode_stats")(None, None, None) == -1


def _bind(L, name, restype):
    f = getattr(L, name)
    f.restype = restype
    return f


def test_no_cpu_fallback_and_loud_failure():
    import torch
    import custom_gymnasium_environments_amd as cge
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(cge.NativeLibraryError):
        cge.SnakeVectorEnv(8, grid_size=10)
    with pytest.raises(cge.NativeLibraryError):
        cge.SnakeVectorEnv(8, grid_size=10, device="cpu")
    for name in ["Crypto", "Traffic", "Parking", "Climate", "Fleet", "Manufacturing", "Hospital"]:     # every env type: no silent CPU path
        with pytest.raises(cge.NativeLibraryError):
            getattr(cge, name + "VectorEnv")(8)
        with pytest.raises(cge.NativeLibraryError):
            getattr(cge, name + "VectorEnv")(8, device="cpu")


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "custom_gymnasium_environments_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "orc_" not in text, f


def test_registry_covers_the_reference_ids():
    """The ids the reference registers with gymnasium / RLlib (file:line in custom_gymnasium_environments_amd/registry.py) resolve
    to the batched classes; an unknown id is an error, not a fallback."""
    import custom_gymnasium_environments_amd as cge
    assert cge.registered_ids() == sorted(["snake_env_classic-v0", "CryptoTrading-v0", "TrafficManagement-v0", "SmartParkingEnv-v0",
                                           "SmartClimateEnv-v0", "FleetManagement-v0", "HospitalManagement-v0", "SmartManufacturing-v0"])
    with pytest.raises(ValueError):
        cge.make_vec("CartPole-v1", 4)
    for name in ["reset", "step", "close", "call", "get_attr", "set_attr", "render", "unwrapped"]:
        assert hasattr(cge.NumpyVectorEnv, name), name
