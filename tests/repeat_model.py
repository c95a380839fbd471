"""Shared by test_repeat_host.py and test_gpu_repeat.py: a NumPy / Python-float model of the
action-repeat rule of include/f110.h ("action repeat"), written out from the contract and
independently of the library, with one loop per env.  The seeded step sequences, the bit
comparison, the row stacking, the NumPy ring and the n-step model come from nstep_model.py."""
import numpy as np

from nstep_model import Model, Ring, same_bits, scenario, stack_rows  # noqa: F401 (re-exported)


class RepeatModel:
    """Per env: a phase k, a running return as a Python float (an IEEE double; a product and a sum
    are two roundings), the latched observation and action; the power table as sequential
    products."""

    def __init__(self, N, K, gamma):
        self.N, self.K = N, K
        self.pw = [1.0]
        for _ in range(K):
            self.pw.append(self.pw[-1] * float(gamma))
        self.k = [0] * N
        self.ret = [0.0] * N
        self.s = [None] * N
        self.a = [None] * N
        # what the runs met (the coverage asserts of the tests)
        self.full = self.by_term = self.by_trunc = self.dropped = self.held = 0

    def hold(self, obs, act):
        """Returns (the action rows the env steps with, the decision mask)."""
        out = np.array(act, np.float32)
        decision = np.zeros(self.N, np.uint8)
        for e in range(self.N):
            if self.k[e] == 0:
                self.s[e], self.a[e] = obs[e].copy(), act[e].copy()
                decision[e] = 1
            else:
                out[e] = self.a[e]
                self.held += 1
        return out, decision

    def push(self, r, s2, term, trunc, reset):
        """Returns the emitted rows [(obs, act, reward f32, next_obs, done f32)], env ascending."""
        rows = []
        pw = self.pw
        with np.errstate(over="ignore"):
            for e in range(self.N):
                if reset[e]:
                    self.dropped += self.k[e] > 0
                    self.k[e] = 0
                    continue
                re = float(r[e])
                if self.k[e] == 0:
                    self.ret[e] = re
                else:
                    p = pw[self.k[e]] * re
                    self.ret[e] = self.ret[e] + p
                self.k[e] += 1
                tr = bool(trunc[e]) if trunc is not None else False
                if term[e] or tr or self.k[e] == self.K:
                    d = np.float32(1.0) if term[e] else np.float32(1.0 - pw[self.k[e] - 1])
                    rows.append((self.s[e], self.a[e], np.float32(self.ret[e]), s2[e], d))
                    if term[e]:
                        self.by_term += 1
                    elif tr:
                        self.by_trunc += 1
                    else:
                        self.full += 1
                    self.k[e] = 0
        return rows

    def phases(self):
        return np.array(self.k, np.int32)

    def returns(self):
        return np.array(self.ret, np.float64)

