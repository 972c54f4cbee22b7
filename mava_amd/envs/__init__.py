from . import cleaner, connector, lbf, rware, smax, spread, synthetic_rware
from .cleaner import Cleaner  # noqa: F401
from .connector import Connector  # noqa: F401
from .lbf import LevelBasedForaging  # noqa: F401
from .rware import RobotWarehouse  # noqa: F401
from .smax import Smax  # noqa: F401
from .spread import Spread  # noqa: F401
from .synthetic_rware import SyntheticRware  # noqa: F401


def make(config, add_global_state: bool = False, device=None, env_offset: int = 0):
    """mava/utils/make_env.py:215-240: (train_env, eval_env) of the configuration's environment.  `env=lbf` builds the
    Level-Based Foraging environment, `env=connector` Connector, `env=cleaner` Cleaner, `env=spread` Spread (this project's
    own continuous-action task; no environment of the reference) and an env group marked `native: true`
    the Robot Warehouse (`env=rware_native`) or SMAX (`env=smax_native`); every other environment name - `env=rware` and
    `env=smax` among them - keeps the synthetic stand-in."""
    if config.env.get("env_name", None) == "LevelBasedForaging":
        mk = lbf.make
    elif config.env.get("env_name", None) == "RobotWarehouse" and bool(config.env.get("native", False)):
        mk = rware.make
    elif config.env.get("env_name", None) == "Smax" and bool(config.env.get("native", False)):
        mk = smax.make
    elif config.env.get("env_name", None) == "MaConnector":
        mk = connector.make
    elif config.env.get("env_name", None) == "Cleaner":
        mk = cleaner.make
    elif config.env.get("env_name", None) == "Spread":
        mk = spread.make
    else:
        mk = synthetic_rware.make
    return mk(config, add_global_state=add_global_state, device=device, env_offset=env_offset)
