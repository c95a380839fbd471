// f110_rays_fxs.hip — k_rays_fxs, the default ray kernel on axis-aligned maps (the hot kernel: ~7
// dependent fp64 gathers per ray): one wave per car, its 64-beam chunks traced in two refilled
// slots on the padded EDT with the fixed-point cell index of f110_rays_fx.h; with other cars in
// the env its leading work items compute the (car, opponent) pair geometry for k_post_multi.
#include <hip/hip_runtime.h>

#include "../../include/f110.h"
#include "f110_beam_runs.h"
#include "f110_math.h"
#include "f110_rays_fx.h"
#include "f110_rng.h"
#include "f110_step_args.h"
#include "f110_step_device.h"

namespace f110 {

// k_rays_fxs: the car's first kRunsLds beam runs sit in a wave-private LDS copy (3-13 runs for
// the default scan), so the per-car run search and every chunk arm read LDS instead of making
// dependent trips to L2 (the runs were written by k_agents just before); runs past kRunsLds (other
// scan configurations) are read from memory as before.
constexpr int kRunsLds = 16;

__device__ __forceinline__ double rfl64(double v) {  // a wave-uniform VGPR double into SGPRs
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// run j's (start, t0, delta) from the LDS copy RL or, past kRunsLds, from RG (j wave-uniform)
__device__ __forceinline__ void run_at(const BeamRun *RL, const BeamRun *RG, int j, int &st, double &t0, double &dl) {
    if (j < kRunsLds) {
        st = __builtin_amdgcn_readfirstlane(RL[j].start);
        t0 = rfl64(RL[j].t0);
        dl = rfl64(RL[j].delta);
    } else {
        st = ld_const(&RG[j].start);
        t0 = ld_const(&RG[j].t0);
        dl = ld_const(&RG[j].delta);
    }
}

// get_scan's theta index of beam bc (laser_models.py:167-184) from the car's runs over the LDS
// copy; lo: the run holding beam b0 (found once per car for all its chunks, see k_rays_fxs)
__device__ __forceinline__ double beam_theta_l(const BeamRun *RL, const BeamRun *RG, int n, int lo, int b0, int bc) {
    int rs;
    double t0, dl;
    run_at(RL, RG, lo, rs, t0, dl);
    for (int j = lo + 1; j < n; ++j) {
        int s2;
        double u0, u1;
        run_at(RL, RG, j, s2, u0, u1);
        if (s2 > b0 + 63) break;
        if (bc >= s2) {
            rs = s2;
            t0 = u0;
            dl = u1;
        }
    }
    return t0 + (double)(bc - rs) * dl;  // get_scan's theta_index (laser_models.py:167-184)
}

__device__ __forceinline__ bool lane_in(uint64_t mask) {
    return (uint32_t)(mask >> (threadIdx.x & 63)) & 1u;
}

// k_rays_fxs's step and cell: the fixed-point offset (the zero cell's
// for an ended ray) and whether the lane lies within the guard band of a cell
// edge (the caller takes the IEEE path for those lanes, both slots at once)
// (kFxsBase: the high dwords of t feed the u24 multiplies directly, the low
// dwords hold the shifted fractions; cx / cy are RayArgs::fxs_cx / fxs_cy)
__device__ __forceinline__ uint32_t fxs_offset_m(const FxLoop &L, double cx, double cy, double &x, double &y,
                                                 double d, double c, double s, uint64_t m, uint32_t zero_v,
                                                 bool &near) {
    x += d * c;  // :135
    y += d * s;  // :136
    double tx, ty;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(tx) : "v"(x), "v"(L.ir), "s"(cx));
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(ty) : "v"(y), "v"(L.ir), "s"(cy));
    near = min(dlo(tx), dlo(ty)) < 2u * kFxsBand;
    const uint32_t prow = __umul24(dhi(ty), L.k1);
    uint32_t fast, off;
    asm volatile("v_mad_u32_u24 %0, %1, 8, %2" : "=v"(fast) : "v"(dhi(tx)), "v"(prow));
    // lanes of the activity mask m take the cell, the others the zero cell: the mask (the slot's
    // ballot, an SGPR pair) is the select's condition as it is, no per-lane copy of it (readfirstlane:
    // the mask is wave-uniform; where the compiler cannot prove it, it must still land in SGPRs)
    // (readfirstlane returns int: each half goes through uint32_t, or the low half would sign-extend)
    const uint64_t ms = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(m >> 32)) << 32) |
                        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)m);
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(off) : "v"(zero_v), "v"(fast), "s"(ms));
    return off;
}

// The leading geometry blocks of k_rays_fxs<HANDOFF>: one lane per (car,
// opponent) pair, from the state k_agents wrote (pre-TTC), beside the ray waves
// instead of on 2-8 lanes of k_post_multi's serial chain.
__device__ __noinline__ void ray_pair_geometry(const RayArgs &a, int blk) {
    const int A = a.A, EA = a.EA;
    const int NP = A - 1;
    const int pr = blk * 64 + (int)(threadIdx.x & 63);  // pair index over the context: car g's pairs g * NP + jj
    if (pr >= EA * NP) return;
    const int g = pr / NP, jj = pr - g * NP;
    const int e = g / A, i = g - e * A;
    const int j = jj < i ? jj : jj + 1;
    const int gj = e * A + j;
    const f110_params &pi = a.pa[i];
    PairGeom &o = a.geo[pr];
    pair_geometry(a.st[g], a.st[EA + g], a.st[(size_t)4 * EA + g], a.st[gj], a.st[EA + gj],
                  a.st[(size_t)4 * EA + gj], pi.length, pi.width, a.B, a.fov, a.beam_incr, o.rv, o.phi, o.wc, o.wh,
                  o.rng);
}

// ------------------------------------------------------------------------
// k_rays_fxs: one wave per car (a.G4 waves per car: wave j takes the car's
// chunks at positions j, j+G4, ... of its chunk order; car-minor block order
// puts car g's waves on XCD g % 8 when EA % 8 == 0).  Its 64-beam chunks are
// traced two at a time in two slots; a slot whose rays have all ended writes
// its chunk's outputs and takes the car's next chunk at once, so both slots
// keep gathers in flight until the car's last chunk (offline model over oracle
// trip counts, scripts/pair_model.py: 146.7k wave-iterations for adjacent
// pairs vs 109.1k).  Padded EDT (kFxsBase offsets), no heavy-first, no masked
// reset; cars whose origin lies off the map trace their chunks one after the
// other with the IEEE cell.  Per ray the arithmetic is k_rays_fxn's, so
// bit-identical.
//
// Chunk order: descending chunk index (the scan's left edge first).  Round 4
// measured two reorderings, both bit-identical and both slower:
// the car's chunk pairs longest first by the previous launch's trips (5 % fewer
// trips, 1-2 % slower), and the blocks' wave items longest first (LPT: the
// indirection costs this 64-VGPR kernel 21 spilled registers).
//
// The refill pass keeps nothing in SGPRs across the loop: kernel arguments
// are re-read at the use through kernarg_here, the scan origin and first
// lookup sit in VGPRs; table loads and the obs store take 32-bit lane offsets
// from an SGPR base.  The obs entry's f32 division by lidar_max is Markstein's
// correction (obs_scan_value_fast).  The arm's (cos, sin) and the finish's
// (side, beam_cos) are one 16-byte load each from the interleaved tables
// RayArgs::cs2 / bs2.
//
// Software-pipelined slots: each slot's gather is waited for right before
// that slot's next step, so one slot's gather is in flight while the other
// slot's data is consumed (the compiler's waits are vmcnt(1): both slots
// gather every trip, a closed slot on the zero cell).  Per slot and trip: the
// total (:141), the activity test (:133), the refill when the slot's chunk has
// ended, the step (:135-136) and its gather.
// LDS: kFxsWaves work items per block with the theta table's (cos, sin) pairs in one LDS copy
// per block: the arms read them there instead of a 16-byte gather each (a wave-level load for the
// texture-address unit, ~24 cycles like a slot gather: 17 per car).  Single-agent
// contexts that share the device with others (f110_set_device_share, the stream sub-shards) take
// it; a lone context keeps one-wave blocks and the gathers, whose launch is shorter (0.685 vs
// 0.697 ms at 65536 cars: the 8-wave blocks hold their LDS until their slowest car ends), as do
// multi-agent contexts (the 8-wave blocks were slower there: C4 one context 27.7 -> 25.2 M).
template <bool HANDOFF, bool LDS, bool COUNT>
__global__ void __launch_bounds__(LDS ? 64 * kFxsWaves : 64, 8) k_rays_fxs(RayArgs a) {  // 8 waves per SIMD: <= 64 VGPRs
    static_assert(!(HANDOFF && LDS), "the LDS table is the single-agent kernel's");
    constexpr int NS = 2;
    constexpr int W = LDS ? kFxsWaves : 1;  // work items (waves) per block
    __shared__ double2 cs_lds[LDS ? kFxsLdsTheta : 1];
    __shared__ BeamRun runs_l[W][kRunsLds];  // each wave's car's first beam runs (kRunsLds)
    const int wave = LDS ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    if (LDS) {  // every load of the block's table copy in flight at once, then the LDS writes
        constexpr int kIt = (kFxsLdsTheta + 64 * W - 1) / (64 * W);
        static_assert(!LDS || kIt * 64 * W == kFxsLdsTheta, "the copy's slots cover the LDS table exactly");
        const double2 *src = reinterpret_cast<const double2 *>(a.cs2);
        double2 v[kIt];
#pragma unroll
        for (int i = 0; i < kIt; ++i) {  // (clamped: every load in bounds and unconditional)
            const int k = (int)threadIdx.x + i * 64 * W;
            v[i] = src[k < a.theta_dis ? k : a.theta_dis - 1];
        }
#pragma unroll
        for (int i = 0; i < kIt; ++i)  // k < kIt * 64 W = kFxsLdsTheta: in bounds (entries >= theta_dis never read)
            cs_lds[(int)threadIdx.x + i * 64 * W] = v[i];
        __syncthreads();
    }
    const int item = (int)blockIdx.x * W + wave;  // the wave's work item
    if (item >= (HANDOFF ? a.geo_blocks : 0) + a.EA * a.G4) return;  // the last block's spare waves
    if (HANDOFF && item < a.geo_blocks) {  // wave-uniform: a geometry item
        ray_pair_geometry(kernarg_here(), item);
        return;
    }
    wave_stamp_start_w(a.wtrace, item);  // (the buffer holds the geometry items too: f110_debug_wave_trace)
    const int bid = HANDOFF ? item - a.geo_blocks : item;  // the ray item (geometry items come first)
    const int wj = bid / a.EA;
    const int g = bid - wj * a.EA;
    const int lane = (int)(threadIdx.x & 63);
    const int B = a.B;
    const int e = HANDOFF ? g / a.A : g;
    const int nch = (B + 63) >> 6;
    const int wstride = a.G4;
    // the chunks whose scans k_post_multi may read (k_agents' handoff_chunks; without it every chunk)
    const uint32_t hmask = HANDOFF ? (a.hmask ? ld_const(a.hmask + g) : 0xFFFFFFFFu) : 0u;
    const double *dt = a.m.dt;
    const FxLoop L = fx_loop(a);
    // Every per-car input is requested before anything waits: the scan origin and first lookup
    // (scalar), the run count, and the LDS copy of the first kRunsLds beam runs (lanes < kRunsLds
    // load whatever the car's run slots hold; only runs < nr are ever read) -- one round trip.
    const double rx = ld_const(a.ray0 + g), ry = ld_const(a.ray0 + a.EA + g), rd = ld_const(a.ray0 + 2 * a.EA + g);
    const int nr = ld_const(a.nruns + g);
    const BeamRun *RG = a.runs + (size_t)g * kMaxSeg;
    BeamRun *RL = runs_l[wave];
    if (lane < kRunsLds) RL[lane] = RG[lane];  // wave-private LDS
    // the scan origin and first lookup in VGPRs (re-arm copies them into a slot)
    double x00, y00, d00;
    asm volatile("v_mov_b64 %0, %1" : "=v"(x00) : "s"(rx));
    asm volatile("v_mov_b64 %0, %1" : "=v"(y00) : "s"(ry));
    asm volatile("v_mov_b64 %0, %1" : "=v"(d00) : "s"(rd));  // :129
    asm volatile("" ::"s"(nr));  // (keeps the run count's load with the others, not sunk into the search)
    uint32_t zero_v;  // the zero cell's offset in a VGPR (the select's other operand is its SGPR mask)
    asm volatile("v_mov_b32 %0, %1" : "=v"(zero_v) : "s"(a.fx_zero));

    // slot r traces chunk kk[r] (-1: closed); lane l owns beam kk[r] * 64 + l
    double x[NS], y[NS], d[NS], tot[NS], c[NS], sn[NS];
    int kk[NS];
    int kpar[NS];         // the noise cache entry of the slot's chunk pair
    int pnext = wj;       // position of this wave's next chunk in the car's chunk order
    int kinfo = 0;        // lane k < nch: the run holding beam 64 k (one divergent search per car)
    uint32_t srch = 0;    // the search's vector loads past the LDS copy (their wave-level count is the max)
    if (nr <= kRunsLds) {  // wave-uniform: the LDS copy holds every run; the last run starting at or
        // before beam 64 lane, by counting (unrolled over the copy: no search loop; lanes >= nch unused)
        int cnt = 0;
#pragma unroll
        for (int j = 1; j < kRunsLds; ++j) cnt += (j < nr && RL[j].start <= lane * 64) ? 1 : 0;
        kinfo = cnt;
    } else if (lane < nch) {
        int lo = 0, hi = nr - 1;
        {
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (RG[mid].start <= lane * 64) lo = mid;
                else hi = mid - 1;
                if (COUNT) ++srch;
            }
        }
        kinfo = lo;
    }
    // wave-level vector loads other than the slot gathers (SIMT / TA accounting, counter 3):
    // the wave's share of the block's table copy (LDS) or the arms' table loads, the finishes'
    // TTC table loads, the guard-band re-gathers (wave-uniform, scalar)
    uint32_t loads = (LDS ? (uint32_t)((a.theta_dis - 64 * wave + 64 * W - 1) / (64 * W)) : 0u) + 2u;  // + the run copy
    uint32_t trips = 0;
    // in_loop: the slot's next `tot += d` completes tot = d (:130)
    auto arm = [&](int r, bool in_loop) {
        const RayArgs &K = kernarg_here();
        const int k = nch - 1 - pnext;
        kpar[r] = (k >> 1) & 1;
        pnext += wstride;
        kk[r] = k;
        const int b = k * 64 + lane, bc = b < B ? b : B - 1;
        const int lo = __builtin_amdgcn_readlane(kinfo, k);
        int ti = (int)beam_theta_l(runs_l[wave], K.runs + (size_t)g * kMaxSeg, ld_const(K.nruns + g), lo, k * 64,
                                   bc);  // :124 (nruns: a scalar-cache hit since the wave's start)
        if (ti >= K.theta_dis) ti = 0;
        double2 t2;
        if (LDS) {
            t2 = cs_lds[ti];
        } else {
            t2 = ld_off(reinterpret_cast<const double2 *>(K.cs2), (uint32_t)ti * 16u);
            if (COUNT) loads = __builtin_amdgcn_readfirstlane(loads + 1u);  // uniform: kept in an SGPR
        }
        c[r] = t2.x;
        sn[r] = t2.y;
        x[r] = x00;
        y[r] = y00;
        d[r] = b < B ? d00 : 0.0;
        tot[r] = in_loop ? 0.0 : d[r];  // :130
    };
    uint32_t lanes = 0;
    // device noise: chunks 2p and 2p + 1 (beams b and b + 64 of a 128-beam block) share one
    // Philox draw (beam_normal_pair_k); the half a finished chunk does not use is kept for its
    // partner in a two-entry cache whose entry alternates from pair to pair in the chunk order
    // (the open pairs are two consecutive ones: the slots take a pair's chunks one after the
    // other), so most pairs are drawn once
    float cval[2] = {0.0f, 0.0f};
    int ctag[2] = {-1, -1};
    auto finish = [&](int r) {  // the ended chunk's outputs (fx_epilogue, noise after the clamp)
        const RayArgs &K = kernarg_here();
        const int b = kk[r] * 64 + lane;
        const bool inb = b < B;
        const int bc = inb ? b : B - 1;
        double nz = 0.0;
        if (K.noise_ext) {
            nz = K.noise_ext[(size_t)e * B + bc];
            if (COUNT) loads = __builtin_amdgcn_readfirstlane(loads + 1u);  // uniform: kept in an SGPR
        } else if (K.noise_std > 0.0) {
            const int pp = kk[r] >> 1, ci = kpar[r];
            float nv;
            if (ctag[ci] == pp) {
                nv = cval[ci];
                ctag[ci] = -1;
            } else {  // the pair index of the unclamped beam: its other half is the partner beam's
                const uint32_t key = noise_key(K.seed, (uint64_t)(K.env_offset + e));
                float lo, hi;
                beam_normal_pair_k(key, ld_const(K.noise_step + e), beam_noise_pair(b), lo, hi);
                nv = (kk[r] & 1) ? hi : lo;
                cval[ci] = (kk[r] & 1) ? lo : hi;
                ctag[ci] = pp;
            }
            nz = K.noise_std * (double)nv;
        }
        if (inb) {  // fx_epilogue
            const double mr = K.max_range;
            double range = tot[r] > mr ? mr : tot[r];  // :143-144
            if (K.noise_ext || K.noise_std > 0.0) range += nz;
            const double v = ld_const(K.vel + g);
            const uint32_t boff = (uint32_t)bc * 8u;
            if (v != 0.0) {
                // the wave loads (side, beam_cos) only when a lane may fire (ttc_may_fire_lane)
                const bool may = ttc_may_fire_lane(range, K.side_max, v, K.ttc_thresh);
                if (__builtin_amdgcn_ballot_w64(may)) {
                    const double2 t2 = ld_off(reinterpret_cast<const double2 *>(K.bs2), boff * 2u);  // (side, beam_cos)
                    if (COUNT) loads = __builtin_amdgcn_readfirstlane(loads + 1u);  // uniform: kept in an SGPR
                    if (may && ttc_fires(range, t2.x, v * t2.y, K.ttc_thresh)) K.ttc_hit[g] = 1;
                }
            }
            if (K.obs && (!HANDOFF || g == e * K.A)) {
                float *orow = K.obs + (size_t)e * K.obs_len;
                *reinterpret_cast<float *>(reinterpret_cast<char *>(orow) + (uint32_t)b * 4u) =
                    obs_scan_value_fast(range, K.lidar_max, K.obs_rinv);
            }
            const size_t row = (size_t)g * B;
            if (K.scans_f32) *reinterpret_cast<float *>(reinterpret_cast<char *>(K.scans_f32 + row) + (uint32_t)b * 4u) = (float)range;
            if (K.scans_f64) *reinterpret_cast<double *>(reinterpret_cast<char *>(K.scans_f64 + row) + (uint32_t)b * 8u) = range;
            if (HANDOFF && ((hmask >> kk[r]) & 1u))
                *reinterpret_cast<double *>(reinterpret_cast<char *>(K.scan + row) + (uint32_t)b * 8u) = range;
        }
        if (COUNT) lanes += (uint32_t)min(64, B - kk[r] * 64);  // the chunk's beams (scalar)
    };

    uint32_t lane_iters = 0, slot_gathers = 0;  // COUNT only
    uint32_t closed_trips = 0;
    const double ux = fma(ld_const(a.ray0 + g), L.ir, L.cxk) - kFxpBase;
    const double uy = fma(ld_const(a.ray0 + a.EA + g), L.ir, L.cyk) - kFxpBase;
    // q + P of the scan origin inside [fxp_lo, fxp_h*): its rays stay in the padded table (false for NaN)
    const bool fast_car = (ux >= a.fxp_lo) & (ux < a.fxp_hx) & (uy >= a.fxp_lo) & (uy < a.fxp_hy);
    if (fast_car) {
#pragma unroll
        for (int r = 0; r < NS; ++r) {
            kk[r] = -1;
            d[r] = tot[r] = x[r] = y[r] = c[r] = sn[r] = 0.0;
        }
#pragma unroll
        for (int r = 0; r < NS; ++r)
            if (pnext < nch) arm(r, true);  // tot = 0: the first trip's total completes tot = d00
        __builtin_amdgcn_s_waitcnt(0);
        // one step of slot r (:133-141): the total, the activity mask, the refill when the slot's
        // chunk has ended (a slot with no chunk left to arm closes: kk = -1, m = 0), the step and its
        // gather.  The mask (two ballots of the bare compares: their AND is one SALU op) selects the
        // gather's offset itself; an ended lane reads the zero cell.  The lookup / lane-slot
        // counters exist in the COUNT build only.
        uint64_t nb[NS];
        auto slot_step = [&](int r) {
            tot[r] += d[r];  // :141 (d00 for a freshly armed slot: tot = d00, :130)
            uint64_t m = __builtin_amdgcn_ballot_w64(dhi(d[r]) != 0u) & __builtin_amdgcn_ballot_w64(tot[r] <= L.mr);
            if (!m && kk[r] >= 0) {  // wave-uniform, rare: the slot's chunk has ended; refill it
                finish(r);
                if (pnext < nch) {
                    arm(r, false);  // tot = d = d00
                    m = __builtin_amdgcn_ballot_w64(dhi(d[r]) != 0u) & __builtin_amdgcn_ballot_w64(tot[r] <= L.mr);
                } else {
                    kk[r] = -1;
                }
                // the refill's own loads (tables) land here, so that the common path's wait
                // before the step stays vmcnt(1) (the other slot's gather may be in flight)
                __builtin_amdgcn_s_waitcnt(0);
            }
            if (COUNT) {
                lane_iters += (uint32_t)__popcll(m);
                ++slot_gathers;
            }
            bool near;
            const uint32_t off = fxs_offset_m(L, a.fxs_cx, a.fxs_cy, x[r], y[r], d[r], c[r], sn[r], m, zero_v, near);
            d[r] = ld_off(dt, off);
            nb[r] = __builtin_amdgcn_ballot_w64(near) & m;
            // nothing of the next slot's step moves above this gather: its total waits for the
            // next slot's own gather (vmcnt(1)), which would otherwise become vmcnt(0) here
            __builtin_amdgcn_sched_barrier(0);
        };
        // the lanes of nb[r] (within the guard band of a cell edge) re-gather slot r's cell from the
        // IEEE cell index (exec-masked, rare); the load lands before the slot's next step (loads
        // return in order)
        auto regather = [&](int r) {
            const RayArgs &K = kernarg_here();
            if (lane_in(nb[r])) d[r] = ld_off(dt, exact_offset_pad(K.m, x[r], y[r], (uint32_t)K.fxp_P));
            if (COUNT) loads = __builtin_amdgcn_readfirstlane(loads + 1u);  // uniform: kept in an SGPR
        };
        // Both slots open: two gathers in flight per trip until a slot closes (its chunk has
        // ended with none of the car's chunks left to arm; in that trip it gathers the zero cell
        // once more).  Then the open slot runs alone.  One guard-band test per trip
        // covers both slots' gathers.
        if (kk[1] >= 0) {
            for (;;) {
#pragma unroll
                for (int r = 0; r < NS; ++r) slot_step(r);
                if (nb[0] | nb[1]) {
                    if (nb[0]) regather(0);
                    if (nb[1]) regather(1);
                    // slot 0's re-gather was issued after slot 1's gather: wait for both here, so
                    // that the common path's wait before slot 0's next step stays vmcnt(1)
                    __builtin_amdgcn_s_waitcnt(0);
                }
                if (COUNT) ++trips;
                if ((kk[0] < 0) | (kk[1] < 0)) break;
            }
            if (kk[0] < 0) {  // the open slot moves into slot 0 (wave-uniform copies)
                x[0] = x[1];
                y[0] = y[1];
                d[0] = d[1];
                tot[0] = tot[1];
                c[0] = c[1];
                sn[0] = sn[1];
                kk[0] = kk[1];
                kpar[0] = kpar[1];
            }
        }
        while (kk[0] >= 0) {  // one slot left
            slot_step(0);
            if (nb[0]) regather(0);
            if (COUNT) {
                ++trips;
                ++closed_trips;
            }
        }
    } else {  // an origin off the map: the IEEE cell of every lookup, chunk after chunk
        uint32_t cnt = 0;
        while (pnext < nch) {
            arm(0, false);
            const RayArgs &K = kernarg_here();
            uint32_t cc = 0;
            while ((dhi(d[0]) != 0u) & (tot[0] <= L.mr)) {
                x[0] += d[0] * c[0];  // :135
                y[0] += d[0] * sn[0];  // :136
                d[0] = ld_off(dt, exact_offset_pad(K.m, x[0], y[0], (uint32_t)K.fxp_P));
                tot[0] += d[0];  // :141
                ++cc;
            }
            cnt += cc;
            if (COUNT) trips += wave_max(cc);  // the chunk's wave-level gathers
            finish(0);
        }
        if (COUNT) {
            lane_iters = wave_sum(cnt);
            slot_gathers = trips;
        }
    }
    if (COUNT) {
        if (lane == 0) {
            const RayArgs &K = kernarg_here();
            unsigned long long *cs = K.ctr + (size_t)(item % kCtrSlots) * kCtrStride;
            atomicAdd(cs, (unsigned long long)(lanes + lane_iters));  // the first lookup came from k_agents
            atomicAdd(cs + 1, (unsigned long long)lanes);
            // lane slots of the gathers the loop issued: 64 per wave-level gather, the ended lanes'
            // zero-cell reads included (SIMT = loop lookups / lane slots); counter 5: trips a slot
            // spent alone (the other one closed)
            atomicAdd(cs + 2, (unsigned long long)slot_gathers * 64ull);
            atomicAdd(cs + 3, (unsigned long long)loads);
            atomicAdd(cs + 5, (unsigned long long)closed_trips);
        }
        const uint32_t ws = wave_max(srch);  // the run search's wave-level loads (counter 3)
        if (lane == 0) atomicAdd(a.ctr + (size_t)(item % kCtrSlots) * kCtrStride + 3, (unsigned long long)ws);
    }
    wave_stamp_end_w(a.wtrace, item, (uint32_t)(trips < 0xffffu ? trips : 0xffffu) << 8 | (uint32_t)wj, (uint32_t)g);
}

// Every k_rays_fxs the library instantiates is named here: <HANDOFF, LDS, COUNT>: single-agent,
// single-agent with the LDS theta table, multi-agent; each with and without the counters.
RayKernel fxs_ray_kernel(const RayPlan &p) {
    static const RayKernel fn[2][3] = {
        {k_rays_fxs<false, false, false>, k_rays_fxs<false, true, false>, k_rays_fxs<true, false, false>},
        {k_rays_fxs<false, false, true>, k_rays_fxs<false, true, true>, k_rays_fxs<true, false, true>}};
    return fn[p.count][p.lds ? 1 : p.handoff ? 2 : 0];
}

}  // namespace f110
