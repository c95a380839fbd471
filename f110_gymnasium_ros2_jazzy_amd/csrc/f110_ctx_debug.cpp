// f110_ctx_debug.cpp — the diagnostic surface of a context (include/f110_debug.h and the counter /
// profiler calls of include/f110.h): every f110_debug_* knob, the lookup / ray counters,
// f110_profile_* and the wave trace.  No step goes through this file.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/f110.h"
#include "../../include/f110_debug.h"
#include "f110_ctx.h"
#include "f110_host_util.h"
#include "f110_step_args.h"

using namespace f110;

// ------------------------------------------------------------ ray knobs ----
extern "C" int f110_debug_ray_kernel(const f110_ctx *ctx) {
    if (!ctx) return fail(F110_E_INVALID, "f110_debug_ray_kernel: null context");
    const int f = plan_ray_launch(ray_knobs(ctx, true), /*masked=*/false).family;
    return f == F110_RAY_TILED_FLAT ? 1 : f == F110_RAY_TILED_CHUNKED ? 2 : 3;
}

extern "C" int f110_debug_ray_lanes(const f110_ctx *ctx) {
    if (!ctx) return fail(F110_E_INVALID, "f110_debug_ray_lanes: null context");
    const int f = plan_ray_launch(ray_knobs(ctx, true), /*masked=*/false).family;
    return f >= F110_RAY_FXN_CLAMPED ? 2 : 1;
}

// k_rays_fxs's waves per car for unmasked steps
extern "C" int f110_debug_ray_refill(const f110_ctx *ctx) {
    if (!ctx) return fail(F110_E_INVALID, "f110_debug_ray_refill: null context");
    const RayPlan p = plan_ray_launch(ray_knobs(ctx, true), /*masked=*/false);
    return p.family == F110_RAY_FXS ? p.G4 : 0;
}

// The one coupling between the knobs: waves > 0 also turns heavy-first off (k_rays_fxs takes no
// heavy-first list) and builds the padded table it reads.  Every other setter writes its own knob only.
extern "C" int f110_debug_set_ray_refill(f110_ctx *ctx, int32_t waves) {
    if (!ctx) return fail(F110_E_INVALID, "f110_debug_set_ray_refill: null context");
    if (waves < 0 || waves > 16) return fail(F110_E_INVALID, "f110_debug_set_ray_refill: waves must be in 0..16");
    const bool fx = ctx->ray_kernel == 3;
    if (!fx && waves != 0) return fail(F110_E_INVALID, "f110_debug_set_ray_refill: this context's ray kernel has no refill");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    ctx->fx_refill = waves;
    if (waves > 0) {
        ctx->heavy_off = true;
        return ensure_padded_table(ctx);  // the padded table goes with k_rays_fxs
    }
    return F110_OK;
}

extern "C" int f110_debug_disable_heavy_first(f110_ctx *ctx) {
    if (!ctx) return fail(F110_E_INVALID, "f110_debug_disable_heavy_first: null context");
    ctx->heavy_off = true;
    return F110_OK;
}

extern "C" int f110_debug_set_ray_lanes(f110_ctx *ctx, int32_t n) {
    if (!ctx) return fail(F110_E_INVALID, "f110_debug_set_ray_lanes: null context");
    if (n < 1 || n > 2) return fail(F110_E_INVALID, "f110_debug_set_ray_lanes: n must be 1 or 2");
    if (ctx->launch_n != 0)
        return fail(F110_E_INVALID, "f110_debug_set_ray_lanes: call before the first reset/step (heavy-first state is per group)");
    const bool fx = ctx->ray_kernel == 3;
    if (!fx && n != 1) return fail(F110_E_INVALID, "f110_debug_set_ray_lanes: this context's ray kernel traces one ray per lane");
    if (fx) ctx->fx_ilp = n;
    return F110_OK;
}

extern "C" int f110_debug_set_ray_gate(f110_ctx *ctx, void *wait_event, void *record_event) {
    if (!ctx) return fail(F110_E_INVALID, "f110_debug_set_ray_gate: null context");
    ctx->gate_wait = static_cast<hipEvent_t>(wait_event);
    ctx->gate_record = static_cast<hipEvent_t>(record_event);
    return F110_OK;
}

extern "C" int f110_debug_set_simt(f110_ctx *ctx, int32_t on) {
    if (!ctx) return fail(F110_E_INVALID, "f110_debug_set_simt: null context");
    ctx->count_slots = on != 0;
    return F110_OK;
}

extern "C" int f110_debug_set_handoff_check(f110_ctx *ctx, int32_t mode) {
    if (!ctx || mode < 0 || mode > 7) return fail(F110_E_INVALID, "f110_debug_set_handoff_check: bad argument");
    ctx->hcheck = mode;
    return F110_OK;
}

// ------------------------------------------------------------- counters ----
// The counter slots on the host, after the stream's work.
static int read_ctr(f110_ctx *ctx, void *stream, std::vector<unsigned long long> &h) {
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    h.resize((size_t)kCtrSlots * kCtrStride);
    HIP_TRY(hipMemcpyAsync(h.data(), ctx->ctr, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return F110_OK;
}

static unsigned long long ctr_sum(const std::vector<unsigned long long> &h, int idx) {
    unsigned long long v = 0;
    for (int i = 0; i < kCtrSlots; ++i) v += h[(size_t)i * kCtrStride + idx];
    return v;
}

extern "C" int f110_read_counters(f110_ctx *ctx, uint64_t *lookups, uint64_t *rays, void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_read_counters: null context");
    std::vector<unsigned long long> h;
    const int rc = read_ctr(ctx, stream, h);
    if (rc != F110_OK) return rc;
    if (lookups) *lookups = ctr_sum(h, 0);
    if (rays) *rays = ctr_sum(h, 1);
    return F110_OK;
}

extern "C" int f110_debug_read_counter(f110_ctx *ctx, int32_t idx, uint64_t *value, void *stream) {
    if (!ctx || !value || idx < 0 || idx >= kCtrStride) return fail(F110_E_INVALID, "f110_debug_read_counter: bad argument");
    std::vector<unsigned long long> h;
    const int rc = read_ctr(ctx, stream, h);
    if (rc != F110_OK) return rc;
    *value = ctr_sum(h, idx);
    return F110_OK;
}

extern "C" int f110_debug_read_simt(f110_ctx *ctx, uint64_t *loop_lookups, uint64_t *lane_slots, void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_debug_read_simt: null context");
    std::vector<unsigned long long> h;
    const int rc = read_ctr(ctx, stream, h);
    if (rc != F110_OK) return rc;
    if (loop_lookups) *loop_lookups = ctr_sum(h, 0) - ctr_sum(h, 1);  // the first lookup of every ray is k_agents'
    if (lane_slots) *lane_slots = ctr_sum(h, 2);
    return F110_OK;
}

extern "C" int f110_reset_counters(f110_ctx *ctx, void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_reset_counters: null context");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    HIP_TRY(hipMemsetAsync(ctx->ctr, 0, (size_t)kCtrSlots * kCtrStride * sizeof(unsigned long long),
                           (hipStream_t)stream));
    return F110_OK;
}

// ------------------------------------------------------------- profiler ----
extern "C" int f110_profile_begin(f110_ctx *ctx, int32_t max_steps) {
    if (!ctx || max_steps < 0) return fail(F110_E_INVALID, "f110_profile_begin: bad arguments");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    ctx->free_prof();
    ctx->prof_ev.resize((size_t)6 * max_steps);
    for (size_t i = 0; i < ctx->prof_ev.size(); ++i) {
        // the events go with the kernels' own dispatches (hipExtLaunchKernel in launch_env_step):
        // each pair holds that kernel's begin / end timestamps, as rocprofv3's kernel trace does,
        // and no marker packet (nor its cache release) sits between the step's kernels
        hipError_t e = hipEventCreateWithFlags(&ctx->prof_ev[i], hipEventDisableSystemFence);
        if (e != hipSuccess) {
            ctx->prof_ev.resize(i);
            ctx->free_prof();
            return hip_fail("hipEventCreate", e);
        }
    }
    ctx->prof_max = max_steps;
    ctx->prof_n = 0;
    return F110_OK;
}

extern "C" int f110_debug_profile_stamps(f110_ctx *ctx, void *ref_event, double *out, int32_t max_steps,
                                         int32_t *steps_out) {
    if (!ctx || !ref_event || !out || max_steps < 0)
        return fail(F110_E_INVALID, "f110_debug_profile_stamps: bad arguments");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    const int n = ctx->prof_n < max_steps ? ctx->prof_n : max_steps;
    for (int i = 0; i < n; ++i) {
        hipEvent_t *ev = &ctx->prof_ev[(size_t)6 * i];
        HIP_TRY(hipEventSynchronize(ev[5]));
        for (int k = 0; k < 6; ++k) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, static_cast<hipEvent_t>(ref_event), ev[k]));
            out[(size_t)6 * i + k] = ms;
        }
    }
    if (steps_out) *steps_out = n;
    return F110_OK;
}

extern "C" int f110_profile_end(f110_ctx *ctx, double ms_out[3], int32_t *steps_out) {
    if (!ctx) return fail(F110_E_INVALID, "f110_profile_end: null context");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    double acc[3] = {0, 0, 0};
    for (int i = 0; i < ctx->prof_n; ++i) {
        hipEvent_t *ev = &ctx->prof_ev[(size_t)6 * i];
        HIP_TRY(hipEventSynchronize(ev[5]));
        for (int k = 0; k < 3; ++k) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
            acc[k] += ms;
        }
    }
    if (ms_out)
        for (int k = 0; k < 3; ++k) ms_out[k] = acc[k];
    if (steps_out) *steps_out = ctx->prof_n;
    ctx->free_prof();
    return F110_OK;
}

// ----------------------------------------------------------- wave trace ----
extern "C" int f110_debug_wave_trace(f110_ctx *ctx, int32_t arm, uint64_t *host_out, int64_t max_waves,
                                     int64_t *n_waves, void *stream) {
    if (!ctx) return fail(F110_E_INVALID, "f110_debug_wave_trace: null context");
    if (use_device(ctx) != F110_OK) return F110_E_HIP;
    const int64_t EA = (int64_t)ctx->cfg.n_envs * ctx->cfg.n_agents;
    // an upper bound of any ray launch's waves (one-wave blocks: the chunked grids' EA x nch
    // plus the heavy-first prefix; k_rays_fxs: EA x waves per car <= EA x nch, after the multi-agent
    // launch's leading geometry items, ceil(EA (A - 1) / 64) rounded up to 8)
    const int64_t geo_items = ctx->cfg.n_agents > 1 ? ((EA * (ctx->cfg.n_agents - 1) + 63) / 64 + 7) / 8 * 8 : 0;
    const int64_t waves = EA * ((ctx->cfg.n_beams + 63) / 64) + ctx->heavy_cap + 64 + geo_items;
    if (!ctx->wtrace) {
        const hipError_t e = ctx->arena.alloc(&ctx->wtrace, (size_t)waves * 4, /*zero=*/true);
        if (e != hipSuccess) return hip_fail("hipMalloc(&q, (size_t)waves * 4 * sizeof(uint64_t))", e);
        ctx->wtrace_n = waves;
    }
    if (n_waves) *n_waves = waves;
    if (host_out) {
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        const int64_t n = max_waves < waves ? max_waves : waves;
        HIP_TRY(hipMemcpy(host_out, ctx->wtrace, (size_t)n * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (arm) HIP_TRY(hipMemsetAsync(ctx->wtrace, 0, (size_t)waves * 4 * sizeof(uint64_t), (hipStream_t)stream));
    ctx->wtrace_armed = arm != 0;
    return F110_OK;
}
