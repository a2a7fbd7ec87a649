"""ctypes binding of libcge_amd.so (the C ABI declared in include/cge_amd.h).

There is deliberately NO fallback: if the HIP library is missing or fails to load, importing an
env class still works (so the package can be inspected on a CPU box) but creating one raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CGE_AMD_LIBRARY: A/B measurements against another build of the SAME library (tools/ab/); not a backend switch
LIB_PATH = os.environ.get("CGE_AMD_LIBRARY") or os.path.join(_HERE, "libcge_amd.so")

CGE_OK = 0
STATUS_NAMES = {0: "CGE_OK", -1: "CGE_ERR_INVALID_ARG", -2: "CGE_ERR_HIP", -3: "CGE_ERR_UNSUPPORTED",
                -4: "CGE_ERR_NO_DEVICE"}
AUTORESET_NEXT_STEP, AUTORESET_SAME_STEP, AUTORESET_DISABLED = 0, 1, 2


class NativeLibraryError(RuntimeError):
    pass


class SnakeConfig(C.Structure):
    _fields_ = [("grid_size", C.c_int32), ("max_steps", C.c_int32), ("autoreset_mode", C.c_int32),
                ("reserved", C.c_int32)]


class CryptoConfig(C.Structure):
    _fields_ = [("initial_balance", C.c_double), ("trading_fee_rate", C.c_double), ("slippage_rate", C.c_double),
                ("min_price", C.c_double), ("max_price", C.c_double), ("volatility_base", C.c_double),
                ("market_psychology_factor", C.c_double), ("max_steps", C.c_int32), ("action_type", C.c_int32),
                ("autoreset_mode", C.c_int32), ("reserved", C.c_int32)]


class TrafficConfig(C.Structure):
    _fields_ = [("grid_rows", C.c_int32), ("grid_cols", C.c_int32), ("num_intersections", C.c_int32),
                ("max_vehicles", C.c_int32), ("spawn_rate", C.c_double), ("max_steps", C.c_int32),
                ("autoreset_mode", C.c_int32)]


class ParkingConfig(C.Structure):
    _fields_ = [("max_steps", C.c_int32), ("autoreset_mode", C.c_int32)]


class ClimateConfig(C.Structure):
    _fields_ = [("max_occupancy", C.c_int32), ("episode_minutes", C.c_int32), ("autoreset_mode", C.c_int32), ("reserved", C.c_int32)]


class FleetConfig(C.Structure):
    _fields_ = [("max_timesteps", C.c_int32), ("autoreset_mode", C.c_int32)]


class HospitalConfig(C.Structure):
    _fields_ = [("max_episode_length", C.c_int32), ("autoreset_mode", C.c_int32)]


class ManufacturingConfig(C.Structure):
    _fields_ = [("max_steps", C.c_int32), ("autoreset_mode", C.c_int32)]


class BusConfig(C.Structure):
    _fields_ = [("max_timesteps", C.c_int32), ("autoreset_mode", C.c_int32)]


class WorldBuilderConfig(C.Structure):
    _fields_ = [("grid_size", C.c_int32), ("flatten_obs", C.c_int32), ("autoreset_mode", C.c_int32), ("reserved", C.c_int32)]


class RestaurantConfig(C.Structure):
    _fields_ = [("max_episode_steps", C.c_int32), ("autoreset_mode", C.c_int32)]


class AirlineConfig(C.Structure):
    _fields_ = [("autoreset_mode", C.c_int32), ("reserved", C.c_int32)]


class EmergencyConfig(C.Structure):
    _fields_ = [("autoreset_mode", C.c_int32), ("max_timesteps", C.c_int32)]


class SpaceStationConfig(C.Structure):
    _fields_ = [("autoreset_mode", C.c_int32), ("max_steps", C.c_int32)]


class FarmConfig(C.Structure):
    _fields_ = [("autoreset_mode", C.c_int32), ("max_years", C.c_int32), ("compact_obs", C.c_int32), ("reserved", C.c_int32)]


class Pcg64State(C.Structure):
    """cge_pcg64_state: NumPy's PCG64 bit_generator.state as 40 bytes."""
    _fields_ = [("state_lo", C.c_uint64), ("state_hi", C.c_uint64), ("inc_lo", C.c_uint64), ("inc_hi", C.c_uint64),
                ("has_uint32", C.c_uint32), ("uinteger", C.c_uint32)]


SAMPLE_INDEX, SAMPLE_UNIFORM, SAMPLE_BITS = 0, 1, 2
DTYPE_INT8, DTYPE_INT32, DTYPE_INT64, DTYPE_FLOAT32 = 0, 1, 2, 3
SAMPLER_MAX_K, SAMPLER_MAX_STEPS = 4096, 65535

# name -> (restype, argtypes); also the list tests check against include/cge_amd.h
_vp, _i32, _i64, _u32, _u64, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_size_t
_host_buf = (C.c_int, [_vp, _vp, _vp])                       # (handle, host or device buffer, stream)

# cge_<env>_<name> for every env type; `create` takes the type's own config struct and is added per type below
_SHARED = {
    "destroy": (C.c_int, [_vp]),
    "seed": (C.c_int, [_vp, _vp, _u64, _vp]),
    "reset": (C.c_int, [_vp, _vp, _vp, _vp]),
    "step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rollout": (C.c_int, [_vp, _i32, _vp, _u64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "device_bytes": (_sz, [_vp]),
    "episode_stats": (C.c_int, [_vp, _vp, _vp]),
    "last_error": (C.c_char_p, [_vp]),
    "last_kernel": (C.c_char_p, [_vp]),
}
# what only some types have, by group; a group may replace a shared prototype (climate's two action pointers)
_EXTRAS = {
    "final_obs": {"rollout_final_obs": (C.c_int, [_vp, _vp, _vp, _i64, _vp]), "final_obs_segment": (_i64, [_vp])},
    "final_obs_rows": {},    # the same two under cge_rows_<env>_* (_env_signatures): beside a surface cge_<env>_* that stays as it is
    "state": {"state_bytes": (_sz, [_vp]), "get_state": _host_buf, "set_state": _host_buf},
    "snapshot": {"snapshot_bytes": (_sz, [_vp]), "snapshot_get": _host_buf, "snapshot_set": _host_buf},
    # canonical records packed on the device, under cge_records_<env>_* (_env_signatures): the four record-lane types, beside their snapshots
    "records": {},
    "done_mask": {"done_mask": (C.c_int, [_vp, _vp])},
    "info": {"info": (C.c_int, [_vp, _i32, _vp, _vp])},
    "info_indexed": {"info": (C.c_int, [_vp, _i32, _i32, _vp, _vp])},
    "info64": {"info64": (C.c_int, [_vp, _i32, _vp, _vp])},
    "total_reward": {"total_reward": _host_buf},
    "render_rgb": {"render_rgb": _host_buf},
    "error_count": {"error_count": (_i64, [_vp, _vp])},
    "two_actions": {"step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
                    "rollout": (C.c_int, [_vp, _i32, _vp, _vp, _u64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp])},
}
_ENV_TYPES = {
    "snake": (SnakeConfig, "final_obs info render_rgb state error_count"),
    "crypto": (CryptoConfig, "final_obs info state"),
    "traffic": (TrafficConfig, "final_obs info_indexed total_reward state"),
    "parking": (ParkingConfig, "final_obs info_indexed info64 snapshot"),
    "climate": (ClimateConfig, "two_actions final_obs info snapshot"),
    "fleet": (FleetConfig, "final_obs info snapshot done_mask"),
    "manufacturing": (ManufacturingConfig, "final_obs info snapshot done_mask"),
    "hospital": (HospitalConfig, "final_obs info snapshot done_mask"),
    "bus": (BusConfig, "final_obs_rows info_indexed error_count snapshot"),
    "world_builder": (WorldBuilderConfig, "final_obs_rows info_indexed error_count state"),
    "restaurant": (RestaurantConfig, "final_obs_rows info error_count snapshot"),
    "airline": (AirlineConfig, "info error_count snapshot records"),
    "emergency": (EmergencyConfig, "final_obs_rows info error_count snapshot records"),
    "space_station": (SpaceStationConfig, "final_obs_rows info error_count snapshot records"),
    "farm": (FarmConfig, "final_obs_rows info error_count snapshot records"),
}
_RECORDS = dict(_EXTRAS["state"], pack=(C.c_int, [_vp, _i64, _i64, _vp, _vp]), unpack=(C.c_int, [_vp, _i64, _i64, _vp, _vp]))
_HAVE_DEFAULT_CONFIG = ("crypto", "traffic")         # the two config structs the library fills with the reference's defaults


def _env_signatures(env, config, extras):
    sig = dict(_SHARED, create=(C.c_int, [C.POINTER(config), _i64, C.c_int, _i64, C.POINTER(_vp)]))
    if env in _HAVE_DEFAULT_CONFIG:
        sig["default_config"] = (None, [C.POINTER(config)])
    for group in extras.split():
        sig.update(_EXTRAS[group])
    out = {f"cge_{env}_{name}": proto for name, proto in sig.items()}
    if "final_obs_rows" in extras.split():
        out.update({f"cge_rows_{env}_{name}": proto for name, proto in _EXTRAS["final_obs"].items()})
    if "records" in extras.split():
        out.update({f"cge_records_{env}_{name}": proto for name, proto in _RECORDS.items()})
    return out


SIGNATURES = {
    "cge_version": (C.c_char_p, []),
    "cge_hash_action": (_u32, [_u64, _u64, _u64, _u32, _u32]),
    "cge_pcg64_advance": (C.c_int, [C.POINTER(Pcg64State), _u64, _u64]),
    "cge_sampler_create": (C.c_int, [_i32, _i64, C.POINTER(C.c_double), _i64, _i64, _i64, C.c_int, C.POINTER(_vp)]),
    "cge_sampler_destroy": (C.c_int, [_vp]),
    "cge_sampler_set_state": (C.c_int, [_vp, C.POINTER(Pcg64State), _vp]),
    "cge_sampler_get_state": (C.c_int, [_vp, C.POINTER(Pcg64State), _vp]),
    "cge_sampler_sample": (C.c_int, [_vp, _i64, _vp, _i32, _vp]),
    "cge_sampler_device_bytes": (_sz, [_vp]),
    "cge_sampler_last_error": (C.c_char_p, [_vp]),
    "cge_sampler_last_kernel": (C.c_char_p, [_vp]),
}
for _env, (_config, _extras) in _ENV_TYPES.items():
    SIGNATURES.update(_env_signatures(_env, _config, _extras))

_lib = None


def lib():
    """Load libcge_amd.so once; raise NativeLibraryError (never fall back) if that is impossible."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} not found: build it with `python -m custom_gymnasium_environments_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:
            raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                if os.environ.get("CGE_AMD_LIBRARY"):          # A/B against an older build: entry points added since are simply absent
                    continue
                raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, handle=None, last_error=None, what=""):
    if status == CGE_OK:
        return
    msg = ""
    if handle is not None and last_error is not None:
        raw = last_error(handle)
        msg = raw.decode() if raw else ""
    raise NativeLibraryError(f"{what} failed: {STATUS_NAMES.get(status, status)} {msg}".strip())
