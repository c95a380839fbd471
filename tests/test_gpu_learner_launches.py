"""The explicit learner's launch sequence per update, pinned: which grouped GEMM / weight-gradient
launches, learner heads and Adam launches one DDPG update and the two kinds of TD3 update issue, in
which order, with how many ops each.  A change to the update's structure has to show here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LOW2, HIGH2 = [-0.4189, 0.0], [0.4189, 20.0]
SIZE_QUERIES = ("f110_ddpg_row_blocks",)  # and every *_scratch_floats: they launch nothing


def G(n):  # a grouped GEMM launch of n ops
    return ("gemm", n, False)


def W(n, loss=False):  # a weight-gradient launch of n ops; loss: its finishing launch writes the loss
    return ("wgrad", n, loss)


def H(name):  # a learner head
    return ("f110_" + name, 0, False)


def ADAM(target):  # FlatAdam.step; target: with the soft update of the network's target
    return ("adam+target" if target else "adam", 0, False)


ACTOR_PHASE = [G(2), G(1), H("ddpg_actor_head"), G(1), H("ddpg_q_mean_step"), G(1), H("ddpg_actor_head_bwd"), G(1),
               W(3, True), ADAM(True)]
DDPG = [G(3), G(2), H("ddpg_actor_head"), G(1), H("ddpg_critic_step"), G(1), W(4, True), ADAM(True)] + ACTOR_PHASE
TD3_CRITIC = [G(3), G(2), G(3), H("td3_target_action"), G(2), H("td3_critic_step"), G(2), W(4), W(4, True)]
TD3_CRITIC_ONLY = TD3_CRITIC + [ADAM(False)]
TD3_ACTOR_STEP = TD3_CRITIC + [ADAM(True)] + ACTOR_PHASE


class _Heads:
    """The library handle with every f110_* launch it is asked for written to ``log``."""

    def __init__(self, L, log):
        self._L, self._log = L, log

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("f110_") or name.endswith("_scratch_floats") or name in SIZE_QUERIES:
            return fn

        def call(*a):
            self._log.append((name, 0, False))
            return fn(*a)
        return call


def _recorded(monkeypatch, algo):
    import f110_gymnasium_ros2_jazzy_amd.ddpg as Dd
    from f110_gymnasium_ros2_jazzy_amd import learner_fused
    log = []
    gemm, wgrad, step = learner_fused.lg.gemm, learner_fused.lg.wgrad, Dd.FlatAdam.step

    def rec_gemm(ops, M, device):
        log.append(("gemm", len(ops), False))
        return gemm(ops, M, device)

    def rec_wgrad(ops, M, device, loss=None):
        log.append(("wgrad", len(ops), loss is not None))
        return wgrad(ops, M, device, loss=loss)

    def rec_step(self, flat_grad, target=None, tau=0.0):
        log.append(ADAM(target is not None))
        return step(self, flat_grad, target, tau)
    monkeypatch.setattr(learner_fused.lg, "gemm", rec_gemm)
    monkeypatch.setattr(learner_fused.lg, "wgrad", rec_wgrad)
    monkeypatch.setattr(Dd.FlatAdam, "step", rec_step)
    ln = Dd.DDPGLearner(obs_dim=12, act_dim=2, action_low=LOW2, action_high=HIGH2, seed=1, device="cuda:0",
                        replay=None, algo=algo, policy_delay=2)
    assert ln.explicit is not None
    ln.explicit.L = _Heads(ln.explicit.L, log)
    return ln, log


def _batch(M=64, D=12):
    g = torch.Generator(device="cuda").manual_seed(M + D)
    S = torch.randn(M, D, device="cuda", generator=g)
    A = torch.rand(M, 2, device="cuda", generator=g) * torch.tensor([0.8378, 20.0], device="cuda") - \
        torch.tensor([0.4189, 0.0], device="cuda")
    R = torch.randn(M, device="cuda", generator=g)
    S2 = S + 0.1 * torch.randn(M, D, device="cuda", generator=g)
    Dn = (torch.rand(M, device="cuda", generator=g) < 0.1).float()
    return S, A, R, S2, Dn, torch.rand(M, device="cuda", generator=g) + 0.5


def test_ddpg_update_launches(gpu, monkeypatch):
    ln, log = _recorded(monkeypatch, "ddpg")
    st = ln.update(*_batch())
    assert log == DDPG
    assert torch.isfinite(st["critic_loss"]) and torch.isfinite(st["actor_loss"])


def test_td3_update_launches(gpu, monkeypatch):
    """policy_delay 2: a critic-only update, then an actor step."""
    ln, log = _recorded(monkeypatch, "td3")
    batch = _batch()
    st = ln.update(*batch)
    assert log == TD3_CRITIC_ONLY and st["actor_loss"] is None
    del log[:]
    st = ln.update(*batch)
    assert log == TD3_ACTOR_STEP
    assert torch.isfinite(st["critic_loss"]) and torch.isfinite(st["actor_loss"])
