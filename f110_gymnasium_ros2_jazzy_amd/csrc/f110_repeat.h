// f110_repeat.h — action repeat: the per-env block rule (its device views and launchers are in
// f110_learner_args.h, next to the n-step window's).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f110_math.h"

namespace f110 {

constexpr int kRepeatMax = 64;

// One env's push into its action-repeat block (the semantics of include/f110.h, "action repeat";
// k_repeat_update and f110_host_repeat_push both call it).  k is the env's phase (rewards in ret,
// 0: a decision is due), ret the block's running return (f64), pw[i] = gamma^i as sequential
// products (pw[0] = 1), r this step's reward.  Returns 1 when the block leaves -- it has its
// `repeat` rewards or the episode ends -- with e_reward = (float)ret and e_done the effective done
// 1 - gamma^(k-1) (1 - done); 0 otherwise (the block goes on, or a reset row dropped it).
F110_HD int repeat_update(int repeat, const double *pw, double r, int term, int trunc, int was_reset, int32_t &k,
                          double &ret, float &e_reward, float &e_done) {
    if (was_reset) {  // not a transition: the block belongs to an episode that is over
        k = 0;
        return 0;
    }
    if (k == 0) {
        ret = r;  // assigned, not 0.0 + r: -0.0 survives
    } else {
        const double p = pw[k] * r;  // (product and sum kept apart: no FMA)
        ret = ret + p;
    }
    k += 1;
    if (term || trunc || k == repeat) {
        e_reward = (float)ret;
        e_done = term ? 1.0f : (float)(1.0 - pw[k - 1]);
        k = 0;
        return 1;
    }
    return 0;
}

}  // namespace f110
