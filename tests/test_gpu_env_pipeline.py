"""F110VectorEnv's step pipeline: step() and step_transition() are one pipeline (same seed, same
actions: the same observations, rewards, flags and statistics bit for bit, with and without the
track observation), and the f110_* entry points one reset(), one step() and one step_transition()
call, in order, pinned for the plain gap-follow env and for the env with everything on."""
import json

import numpy as np
import pytest
import torch

import pursuit_cases as C

pytestmark = pytest.mark.gpu

STEPS = 20


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def track(gpu):
    from f110_gymnasium_ros2_jazzy_amd.reward import CenterlineTrack
    tr = CenterlineTrack(C.spielberg_xy()[0], closed=True, device=0)
    yield tr
    tr.close()


def _full_env(track, gpu, track_obs):
    """Four two-agent envs racing the waypoint follower with every per-step stage on: their own
    reward function, a time limit of 7 steps, episode and race statistics."""
    from f110_gymnasium_ros2_jazzy_amd.reward import BatchedCenterlineReward
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    rf = BatchedCenterlineReward(4, dt=0.01, progress=track, device=gpu)
    return F110VectorEnv(4, num_agents=2, opponent="pure_pursuit", opponent_track=track, opponent_speed=3.0, seed=5,
                         device=0, reward_fn=rf, episode_stats=True, race_stats=True, max_episode_steps=7,
                         infos="minimal", **(dict(track_obs=True) if track_obs else {}))


@pytest.mark.parametrize("track_obs", [True, False])
def test_step_and_step_transition_are_one_pipeline(gpu, track, track_obs):
    eager, trans = _full_env(track, gpu, track_obs), _full_env(track, gpu, track_obs)
    try:
        o0, _ = eager.reset(seed=9)
        o1, _ = trans.reset(seed=9)
        assert same_bits(o0, o1) and o0.shape == (4, 1088 + (20 if track_obs else 0))
        rng = np.random.default_rng(1)
        resets = 0
        for k in range(STEPS):
            a = torch.as_tensor(np.stack([rng.uniform(-0.3, 0.3, 4), rng.uniform(1.0, 6.0, 4)], 1).astype(np.float32),
                                device=gpu)
            obs, rew, term, trunc, info = eager.step(a)
            t_obs, t_rew, t_term, t_reset = trans.step_transition(a)
            assert same_bits(t_obs, obs), f"obs, step {k}"
            assert torch.equal(t_rew.view(torch.int64), rew.view(torch.int64)), f"rewards, step {k}"
            assert torch.equal(t_term.bool(), term), f"terminated, step {k}"
            assert torch.equal(t_reset.bool(), info["reset"]), f"was_reset, step {k}"
            assert torch.equal(trans.truncated, eager.truncated) and torch.equal(trans.truncated.bool(), trunc), \
                f"truncated, step {k}"
            for name in ("last_return", "last_length"):
                x, y = getattr(eager._episode, name), getattr(trans._episode, name)
                assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                                   y.view(torch.int64) if y.dtype == torch.float64 else y), f"{name}, step {k}"
            for name in ("progress", "lead"):
                x, y = getattr(eager._race, name), getattr(trans._race, name)
                assert torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)), \
                    f"{name}, step {k}"
            assert torch.equal(eager._race.result, trans._race.result), f"result, step {k}"
            resets += int(info["reset"].sum())
        assert resets >= 8  # every env was reset on the device twice
        assert eager.episode_totals() == trans.episode_totals() and eager.episode_totals()["episodes"] >= 8
        assert eager.race_totals() == trans.race_totals() and eager.race_totals()["episodes"] >= 8
    finally:
        eager.close()
        trans.close()


# ---- the per-step call sequence -------------------------------------------------------------
# Recorded at the commit before the two step methods were folded into one pipeline, with this
# test's own body.  (f110_default_pursuit_params: pure_pursuit builds its parameter struct per call.)
SIM_RESET = ["f110_set_reset_dtype", "f110_reset", "f110_set_reset_dtype"]
PLAIN = {
    "reset": SIM_RESET + ["f110_gap_follow", "f110_get_state"],
    "step": ["f110_step", "f110_gap_follow", "f110_get_state"],
    "step_transition": ["f110_step", "f110_gap_follow"],
}
FULL_STEP = ["f110_step", "f110_ctx_track_obs", "f110_default_pursuit_params", "f110_pure_pursuit", "f110_reward",
             "f110_episode_stats", "f110_race_stats"]
FULL = {
    "reset": SIM_RESET + ["f110_ctx_track_obs", "f110_default_pursuit_params", "f110_pure_pursuit", "f110_race_stats"],
    "step": FULL_STEP,
    "step_transition": FULL_STEP,
}


class _Logged:
    """The library handle with every f110_* entry point it is asked for written to ``log`` (the
    pure size queries left out: they launch nothing)."""

    def __init__(self, L, log):
        self._L, self._log = L, log

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("f110_") or name.endswith(("_scratch_bytes", "_scratch_floats", "_width")):
            return fn

        def call(*a):
            self._log.append(name)
            return fn(*a)
        return call


@pytest.mark.parametrize("config", ["plain", "full"])
def test_call_sequence_is_pinned(gpu, monkeypatch, track, config):
    """The entry points of one reset(), one step() and one step_transition() of a fresh env: the
    plain gap-follow env, and the env with everything on."""
    from f110_gymnasium_ros2_jazzy_amd import _lib
    from f110_gymnasium_ros2_jazzy_amd.vector_env import F110VectorEnv
    log = []
    monkeypatch.setattr(_lib, "_lib", _Logged(_lib.load(), log))  # what every _lib.load() now returns
    env = (F110VectorEnv(4, num_agents=2, opponent="gap_follow", seed=5, device=0) if config == "plain"
           else _full_env(track, gpu, True))
    try:
        a = torch.tensor([[0.05, 3.0]] * 4, device=gpu)
        seq = {}
        for name, call in (("reset", lambda: env.reset(seed=3)), ("step", lambda: env.step(a)),
                           ("step_transition", lambda: env.step_transition(a))):
            del log[:]
            call()
            seq[name] = list(log)
        torch.cuda.synchronize()
    finally:
        del log[:]
        env.close()
    print("call sequence:", json.dumps(seq))
    assert seq == (PLAIN if config == "plain" else FULL)
