"""EpisodeStats: per-env episode return / length and running totals on the device.

Thin owner of the buffers f110_episode_stats (include/f110.h) works on: one
call per vector step, on that step's rewards and flags, two small launches on
the current torch stream with no host work -- a captured step graph replays it.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._dev import cuda_device, ptr as P, stream, u8_rows


class EpisodeStats:
    """Episode bookkeeping of ``n_envs`` autoresetting envs.

    ``update(rewards, terminated, truncated, was_reset)`` adds one step: a reset row (NEXT_STEP
    autoreset's reset observation) starts a new episode and its reward is ignored; a row whose
    ``terminated`` or ``truncated`` is set finishes the episode (terminated wins).  ``last_return``
    / ``last_length`` hold each env's last finished episode, ``finished`` the envs that finished
    in the last update; ``totals()`` the running totals over all finished episodes."""

    def __init__(self, n_envs: int, device=0):
        self.L = _lib.load()
        self.device = dev = cuda_device(device, "EpisodeStats")
        self.n_envs = n = int(n_envs)
        self.state = torch.zeros(n, _lib.EPISODE_STATE_BYTES, dtype=torch.uint8, device=dev)
        self.last_return = torch.zeros(n, dtype=torch.float64, device=dev)
        self.last_length = torch.zeros(n, dtype=torch.int32, device=dev)
        self.finished = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._totals = torch.zeros(_lib.EPISODE_TOTALS_BYTES, dtype=torch.uint8, device=dev)
        self._scratch = torch.zeros(int(self.L.f110_episode_scratch_bytes(n)), dtype=torch.uint8, device=dev)

    def reset(self):
        """Every env starts a fresh episode; last_return / last_length / finished are zeroed.  The
        totals stay (reset_totals)."""
        self.state.zero_()
        self.last_return.zero_()
        self.last_length.zero_()
        self.finished.zero_()

    def update(self, rewards, terminated, truncated, was_reset):
        """One step's rows (device tensors: rewards float64 [n], flags u8 / bool [n]; truncated may
        be None).  Asynchronous on the current stream."""
        n = self.n_envs
        r = torch.as_tensor(rewards, device=self.device).reshape(-1)
        if r.dtype != torch.float64 or not r.is_contiguous():
            r = r.to(torch.float64).contiguous()
        if r.shape[0] != n:
            raise ValueError(f"EpisodeStats: rewards must have {n} entries; got {r.shape[0]}")
        te = u8_rows(terminated, n, self.device, "EpisodeStats: terminated")
        tr = u8_rows(truncated, n, self.device, "EpisodeStats: truncated")
        wr = u8_rows(was_reset, n, self.device, "EpisodeStats: was_reset")
        self._keep = (r, te, tr, wr)
        _lib.check(self.L.f110_episode_stats(P(r), P(te), P(tr), P(wr), n, P(self.state), P(self.last_return),
                                             P(self.last_length), P(self.finished), P(self._totals),
                                             P(self._scratch), stream(self.device)), "f110_episode_stats")

    def totals(self) -> dict:
        """The running totals as Python numbers (episodes, terminated, truncated, length_sum,
        return_sum, return_min, return_max; min / max are None before the first episode), plus
        return_mean and length_mean.  Waits for the current stream."""
        raw = self._totals.cpu().numpy().tobytes()
        t = _lib.F110EpisodeTotals.from_buffer_copy(raw).as_dict()
        n = t["episodes"]
        if n == 0:
            t["return_min"] = t["return_max"] = None
        t["return_mean"] = t["return_sum"] / n if n else None
        t["length_mean"] = t["length_sum"] / n if n else None
        return t

    def reset_totals(self):
        self._totals.zero_()


def host_episode_stats(rewards, terminated, truncated, was_reset, state, last_return=None, last_length=None,
                       finished=None, totals=None):
    """f110_host_episode_stats over NumPy arrays (in place): the device's semantics in ascending env
    order.  state: uint8 [n, 16] (f110_episode_state rows); totals: an _lib.F110EpisodeTotals."""
    L = _lib.load()
    n = int(np.asarray(rewards).shape[0])
    for a, dt in ((rewards, np.float64), (terminated, np.uint8), (truncated, np.uint8), (was_reset, np.uint8),
                  (state, np.uint8), (last_return, np.float64), (last_length, np.int32), (finished, np.uint8)):
        if a is not None and (a.dtype != dt or not a.flags.c_contiguous):
            raise ValueError("host_episode_stats: arrays must be C-contiguous float64 / uint8 / int32 as declared")
    _lib.check(L.f110_host_episode_stats(P(rewards), P(terminated), P(truncated), P(was_reset), n, P(state),
                                         P(last_return), P(last_length), P(finished), ctypes.byref(totals)),
               "f110_host_episode_stats")
