"""CryptoVectorEnv — batched drop-in for CryptoTradingEnv (crypto_trading_env/crypto_trading_env.py:224-561)."""
import ctypes as C

import numpy as np
import torch

from . import _native
from ._spaces import Box, Discrete
from .vector_env import DeviceVectorEnv

INFO_FIELDS = {"portfolio_value": 0, "cash": 1, "holdings": 2, "current_price": 3, "market_psychology": 4,
               "regime": 5, "step": 6, "trend_strength": 7, "episodes": 8, "needs_reset": 9, "cash_kind": 10}
REGIME_NAMES = ("bull_run", "bear_market", "sideways", "crash", "recovery")   # MarketRegime, :20-25
OBS_DIM = 261   # actual length of _get_observation() (:505-561); the reference's declared space says 260 (:286)


class CryptoVectorEnv(DeviceVectorEnv):
    """N independent CryptoTradingEnv instances stepped by one HIP kernel launch.

    Spaces: obs float32 (261,) — the length the reference actually returns; actions `Discrete(5)`
    (0 hold, 1 buy 5 %, 2 buy 20 %, 3 sell 5 %, 4 sell 20 %) or `Box(-1, 1, (2,), float32)` when
    action_type="continuous".  reward = portfolio change at the pre-step price, -1 when no trade
    happened (:440-446), returned as float32; terminated when step >= 1000, portfolio <= 0 or
    portfolio >= 10x initial (:382-386); truncated always False.

    RNG protocol: `reset(seed=s)` gives env i both generator families the reference seeds
    (`random.seed(s+i)` and `np.random.seed(s+i)`, :305-307) as private per-env MT19937 streams;
    the market simulator state survives resets, as in the reference (:257).
    """

    _abi = "cge_crypto"
    _seed_bits = 32   # np.random.seed(s_i)
    INFO_FIELDS = INFO_FIELDS
    metadata = {"render_modes": []}

    def __init__(self, num_envs, action_type="discrete", device="cuda:0", autoreset_mode="NextStep", env_index0=0,
                 config=None, max_steps=1000, reuse_buffers=False, info_fields=(), record_episode_statistics=False, reference_info=False):
        self._init_common(num_envs, device, autoreset_mode, env_index0, reuse_buffers)
        if action_type not in ("discrete", "continuous"):
            raise ValueError("action_type must be 'discrete' or 'continuous'")
        self.action_type = action_type
        self.continuous = action_type == "continuous"
        if self.continuous:
            self._action_shape, self._action_dtype = (2,), torch.float32
        cfg = _native.CryptoConfig()
        self._lib.cge_crypto_default_config(C.byref(cfg))
        for k, v in (config or {}).items():    # TradingConfig field names (:28-38)
            if not hasattr(cfg, k):
                raise ValueError(f"unknown or unsupported TradingConfig field {k!r} (history_length is fixed at 50 in this build)")
            setattr(cfg, k, v)
        cfg.max_steps = int(max_steps)
        cfg.action_type = int(self.continuous)
        cfg.autoreset_mode = self._mode_code
        self.single_action_space = Box(-1.0, 1.0, (2,), np.float32) if self.continuous else Discrete(5)
        self.single_observation_space = Box(-np.inf, np.inf, (OBS_DIM,), np.float32)
        self._obs_shape = (self.num_envs, OBS_DIM)
        self._create(cfg, info_fields, record_episode_statistics, reference_info)

    def reference_info(self):
        """The reference's step() `info` dict under ITS keys (crypto_trading_env.py:390-398): portfolio_value, cash, holdings,
        current_price, market_psychology as float64 tensors of length N, and market_regime as int32 codes into REGIME_NAMES
        (the reference puts the enum's string there; `regime_names()` maps a host copy).  `trade_info` (the dict describing
        the step's trade) is not kept on the device and is not reproduced."""
        return {"portfolio_value": self.info("portfolio_value"), "cash": self.info("cash"), "holdings": self.info("holdings"),
                "current_price": self.info("current_price"), "market_regime": self.info("regime").to(torch.int32),
                "market_psychology": self.info("market_psychology")}

    @staticmethod
    def regime_names(codes):
        """MarketRegime values (:20-25) for the int codes in infos["market_regime"] (a host-side convenience)."""
        return np.asarray(REGIME_NAMES, dtype=object)[np.asarray(torch.as_tensor(codes).cpu(), dtype=np.int64)]
