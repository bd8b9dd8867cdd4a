"""CPU: the time limit of the batched step (include/navsim.h navsim_config.max_episode_steps, navsim_step_io.truncated,
ABI 7) -- its place in the C ABI and its keyword on NavGymEnv.  The device behaviour is tests/test_gpu_time_limit.py."""
import copy
import ctypes as C
import pickle

import pytest

from nav_gym_amd import abi


def test_abi_7_layout_and_default():
    from nav_gym_amd import lib
    L = lib.load()
    assert abi.ABI_VERSION == 7 and L.navsim_abi_version() == 7
    cfg = lib.default_config()
    assert cfg.max_episode_steps == 0                      # navsim_default_config's memset: no limit
    # the field sits in the tail padding of navsim_config: the size -- and with it the kernarg offsets of state and io -- stay
    assert abi.NavsimConfig.max_episode_steps.offset == 620
    assert abi.NavsimConfig._fields_[-1][0] == "max_episode_steps"
    assert C.sizeof(abi.NavsimConfig) == 624 == L.navsim_sizeof_config()
    assert abi.NavsimStepIO._fields_[-1][0] == "truncated"
    assert abi.NavsimStepIO.truncated.offset == abi.NavsimStepIO.reset_mask.offset + C.sizeof(C.c_void_p)
    assert C.sizeof(abi.NavsimStepIO) == L.navsim_sizeof_step_io()
    # the flags are an output of their own, allocated only with a limit: what a step returns without one keeps its keys
    assert "truncated" not in abi.IO_LAYOUT and abi.LIMIT_LAYOUT == {"truncated": ("uint8", ("E",))}


def test_env_keyword_reaches_the_config_and_survives_copies():
    import nav_gym_env
    env = nav_gym_env.make("NavGym-v0", num_envs=3, max_episode_steps=7)
    assert env.max_episode_steps == 7 and env.cfg.max_episode_steps == 7
    for twin in (pickle.loads(pickle.dumps(env)), copy.deepcopy(env)):
        assert twin.max_episode_steps == 7 and twin.cfg.max_episode_steps == 7 and twin.num_envs == 3
    plain = nav_gym_env.make("NavGym-v0", num_envs=3)
    assert plain.max_episode_steps is None and plain.cfg.max_episode_steps == 0
    # the registered kwargs stay the reference's: the limit is an override only
    from nav_gym_amd import registry
    assert "max_episode_steps" not in registry.spec("NavGym-v0")["kwargs"]


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "7"])
def test_env_keyword_rejects_what_is_not_a_positive_int(bad):
    import nav_gym_env
    with pytest.raises(ValueError):
        nav_gym_env.make("NavGym-v0", num_envs=3, max_episode_steps=bad)
