// f110_race.h — the row rule of the race statistics (private; include/f110.h, "race statistics"):
// what follows the two cars' projections onto the centerline.  k_race (f110_race.hip) and
// f110_host_race_stats (f110_task_capi.cpp) both call it, so the device and the host statement
// differ in nothing but the order the finished envs' sums are added up in.  f64, left to right, no
// FMA (no multiply-add pair below: the direction's product is exact).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/f110.h"
#include "f110_math.h"

namespace f110 {

// f110_race_state.flags
constexpr int32_t kRaceStarted = 1, kRaceClosed = 2, kRaceS0 = 4, kRaceS1 = 8, kRaceAhead = 16, kRaceOppCrashed = 32;
// the result byte
constexpr int kRaceFinished = 1, kRaceEgoCrash = 2, kRaceCompleted = 4, kRaceTruncated = 8, kRaceOppCrash = 16,
              kRaceAheadAtEnd = 32;

static_assert(sizeof(f110_race_params) == 16, "f110_race_params: one double, two int32");
static_assert(sizeof(f110_race_state) == 64, "f110_race_state: six doubles, four int32");
static_assert(sizeof(f110_race_totals) == 112, "f110_race_totals: nine int64, five doubles");

// The arguments f110_race_stats and f110_host_race_stats refuse (F110_E_INVALID), the track and the
// scratch aside.  Written so that a NaN margin fails its test.
inline bool race_bad_args(const f110_race_params *p, const float *ego, int64_t stride, const uint8_t *terminated,
                          const uint8_t *was_reset, int64_t n_envs, const f110_race_state *state,
                          const uint8_t *result, const f110_race_totals *totals) {
    if (!p || !ego || !terminated || !was_reset || !state || !result || !totals) return true;
    if (stride < 4 || n_envs < 0 || n_envs > 0x7fffffffLL) return true;
    if (!(p->pass_margin >= 0.0)) return true;
    return p->direction != 1 && p->direction != -1;
}

// One env's row: the projections of its cars (ok[k] == 0: car k's x or y is not finite, or there
// is no car k; s[k] / t0 are then unused), the collision entries and the three flags.
struct RaceRow {
    double s[2], t0;
    int ok[2], col[2];
    int term, trunc, was_reset, has_opp;
};

F110_HD double race_wrap(double d, int closed, double L) {
    if (closed) {
        if (d > 0.5 * L) d -= L;
        if (d < -0.5 * L) d += L;
    }
    return d;
}

// The lead the state holds: lead0 + (prog[0] - prog[1]), 0 without an opponent.
F110_HD double race_lead(const f110_race_state &st, int has_opp) {
    return has_opp ? st.lead0 + (st.prog[0] - st.prog[1]) : 0.0;
}

// The rule of include/f110.h in its order.  Returns the result byte (0: the env does not finish);
// when it finishes st.prog[0], race_lead(st), st.len, st.t_max, st.passes and st.passed are the
// episode's.
F110_HD int race_update(const f110_race_params &P, int closed, double L, const RaceRow &r, f110_race_state &st) {
    const double dir = (double)P.direction;
    if (r.was_reset || !(st.flags & kRaceStarted)) {  // 1. start row
        st = f110_race_state{};
        st.flags = kRaceStarted;
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (r.ok[k]) {
                st.s_prev[k] = r.s[k];
                st.flags |= kRaceS0 << k;
            }
        if (r.ok[0] && r.ok[1]) st.lead0 = race_wrap(dir * (r.s[0] - r.s[1]), closed, L);
        if (st.lead0 > 0.0) st.flags |= kRaceAhead;
        return 0;
    }
    if (st.flags & kRaceClosed) return 0;  // 2. closed row
#pragma unroll
    for (int k = 0; k < 2; ++k)  // 3. progress
        if (r.ok[k]) {
            if (st.flags & (kRaceS0 << k)) st.prog[k] += dir * race_wrap(r.s[k] - st.s_prev[k], closed, L);
            st.s_prev[k] = r.s[k];
            st.flags |= kRaceS0 << k;
        }
    st.len += 1;
    if (r.ok[0]) {
        const double at = r.t0 < 0.0 ? -r.t0 : r.t0;
        if (at > st.t_max) st.t_max = at;
    }
    double lead = 0.0;
    if (r.has_opp) {  // 4. lead and passes
        if (r.col[1]) st.flags |= kRaceOppCrashed;
        lead = race_lead(st, 1);
        if (!(st.flags & kRaceAhead) && lead > P.pass_margin) {
            st.flags |= kRaceAhead;
            st.passes += 1;
        } else if ((st.flags & kRaceAhead) && lead < -P.pass_margin) {
            st.flags &= ~kRaceAhead;
            st.passed += 1;
        }
    }
    if (!(r.term || r.trunc)) return 0;  // 6.
    st.flags |= kRaceClosed;             // 5. finish
    int res = kRaceFinished;
    if (r.term) res |= r.col[0] ? kRaceEgoCrash : kRaceCompleted;
    else res |= kRaceTruncated;
    if (st.flags & kRaceOppCrashed) res |= kRaceOppCrash;
    if (r.has_opp && lead > 0.0) res |= kRaceAheadAtEnd;
    return res;
}

// The envs finishing in one call (or one block's, or one env's share of them): what the totals add.
// n == 0: empty (prog_mn / prog_mx unused; t_max's neutral element is 0, no |t| is below it).
struct RacePart {
    int64_t n, ego_crashes, completed, truncated, opp_crashes, ahead, passes, passed, len;
    double prog_sum, prog_mn, prog_mx, lead_sum, t_max;
};
static_assert(sizeof(RacePart) == 112, "RacePart: nine int64, five doubles");

F110_HD RacePart race_part_empty() { return RacePart{0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

F110_HD RacePart race_part(int res, const f110_race_state &st, int has_opp) {
    RacePart p = race_part_empty();
    if (res) {
        p.n = 1;
        p.ego_crashes = (res & kRaceEgoCrash) != 0;
        p.completed = (res & kRaceCompleted) != 0;
        p.truncated = (res & kRaceTruncated) != 0;
        p.opp_crashes = (res & kRaceOppCrash) != 0;
        p.ahead = (res & kRaceAheadAtEnd) != 0;
        p.passes = st.passes;
        p.passed = st.passed;
        p.len = st.len;
        p.prog_sum = p.prog_mn = p.prog_mx = st.prog[0];
        p.lead_sum = race_lead(st, has_opp);
        p.t_max = st.t_max;
    }
    return p;
}

// a += b, in this operand order (the fixed summation order is built from it)
F110_HD void race_merge(RacePart &a, const RacePart &b) {
    if (b.n) {
        a.prog_mn = a.n ? (b.prog_mn < a.prog_mn ? b.prog_mn : a.prog_mn) : b.prog_mn;
        a.prog_mx = a.n ? (b.prog_mx > a.prog_mx ? b.prog_mx : a.prog_mx) : b.prog_mx;
    }
    a.n += b.n;
    a.ego_crashes += b.ego_crashes;
    a.completed += b.completed;
    a.truncated += b.truncated;
    a.opp_crashes += b.opp_crashes;
    a.ahead += b.ahead;
    a.passes += b.passes;
    a.passed += b.passed;
    a.len += b.len;
    a.prog_sum += b.prog_sum;
    a.lead_sum += b.lead_sum;
    a.t_max = b.t_max > a.t_max ? b.t_max : a.t_max;
}

F110_HD void race_totals_add(f110_race_totals &t, const RacePart &b) {
    RacePart a = {t.episodes, t.ego_crashes, t.completed, t.truncated, t.opp_crashes, t.ahead_at_end, t.passes,
                  t.passed, t.length_sum, t.progress_sum, t.progress_min, t.progress_max, t.lead_sum, t.t_max};
    race_merge(a, b);
    t.episodes = a.n;
    t.ego_crashes = a.ego_crashes;
    t.completed = a.completed;
    t.truncated = a.truncated;
    t.opp_crashes = a.opp_crashes;
    t.ahead_at_end = a.ahead;
    t.passes = a.passes;
    t.passed = a.passed;
    t.length_sum = a.len;
    t.progress_sum = a.prog_sum;
    t.progress_min = a.prog_mn;
    t.progress_max = a.prog_mx;
    t.lead_sum = a.lead_sum;
    t.t_max = a.t_max;
}

// What k_race_project leaves per env for k_race: each half-wave's first lane writes its own car's
// fields (one writer per element).
struct RaceProj {
    double s0, t0, s1;
    int32_t ok0, ok1;
};
static_assert(sizeof(RaceProj) == 32, "RaceProj: three doubles, two int32");

}  // namespace f110
