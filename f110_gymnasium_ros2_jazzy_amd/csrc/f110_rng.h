// f110_rng.h — the counter-based generators (Philox4x32-10, Philox2x32-10) and what the env draws
// from them: the scan noise's normals and the autoreset spawn choice.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f110_math.h"

namespace f110 {

// ----------------------------------------------------------------- noise --
// Philox4x32-10 (Salmon et al., SC'11) keyed by (seed, global env id);
// counter = (beam pair, steps since reset, stream tag).  Scan noise replaces
// numpy default_rng(seed).normal(0, std, B) (laser_models.py:450-452): same
// stream for every agent of an env and restarted at every reset
// (base_classes.py:119,204), like the reference.
struct U4 { uint32_t x, y, z, w; };

F110_HD U4 philox(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
        U4 n;
        n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
        n.y = (uint32_t)p1;
        n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
        n.w = (uint32_t)p0;
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

F110_HD double u01_open(uint32_t hi, uint32_t lo) {  // (0, 1], 53 bits
    uint64_t v = ((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6);
    return ((double)v + 1.0) * (1.0 / 9007199254740992.0);
}

// Philox2x32-10 (Salmon et al., SC'11; passes BigCrush): one 32x32->64
// multiply and one xor3 per round, half the work of Philox4x32 for the 48
// random bits one normal needs.
struct U2 { uint32_t x, y; };

F110_HD U2 philox2x32(uint32_t L, uint32_t R, uint32_t k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p = (uint64_t)0xD256D193u * L;
        const uint32_t hi = (uint32_t)(p >> 32);
        L = hi ^ k ^ R;
        R = (uint32_t)p;
        k += 0x9E3779B9u;
    }
    return {L, R};
}

// the noise key of (seed, env): distinct envs of one seed get distinct keys
// (an odd multiplier is a bijection mod 2^32)
F110_HD uint32_t noise_key(uint64_t seed, uint64_t env) {
    return (uint32_t)seed ^ ((uint32_t)(seed >> 32) * 0x85EBCA6Bu) ^ ((uint32_t)env * 0x9E3779B9u) ^
           ((uint32_t)(env >> 32) * 0xC2B2AE35u);
}

// N(0,1) noise of the env's stream at `step`: beams b and b + 64 of each
// 128-beam block share one Philox2x32 block (counter (step, p | step_hi <<
// 16) with p = (b >> 7) * 64 + (b & 63), key noise_key(seed, env)) and take
// the two outputs of one Box-Muller transform, rad * cos and rad * sin
// (independent N(0,1)), on 24-bit uniforms in fp32 hardware transcendentals
// (v_log, v_sqrt, v_cos, v_sin: the noise is a statistical quantity, its ~1e-7
// relative precision is far below the 0.01 m std it scales; tails are cut at
// 5.8 sigma).  A lane tracing both beams (k_rays_fxn<2>) draws once for two.
// The key is per env: wave-uniform in the chunked ray kernels.
F110_D void beam_normal_pair_k(uint32_t key, uint64_t step, int p, float &n_lo, float &n_hi) {
    const U2 r = philox2x32((uint32_t)step, (uint32_t)p | ((uint32_t)(step >> 32) << 16), key);
    const float u1 = ((float)(r.x >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
    const float u2 = (float)(r.y >> 8) * (1.0f / 16777216.0f);           // [0, 1)
    const float rad = __builtin_amdgcn_sqrtf(-2.0f * 0.69314718055994531f * __builtin_amdgcn_logf(u1));
    n_lo = rad * __builtin_amdgcn_cosf(u2);  // cos(2 pi u2): beam (b & ~64)
    n_hi = rad * __builtin_amdgcn_sinf(u2);  // sin(2 pi u2): beam (b | 64)
}

F110_D int beam_noise_pair(int b) { return ((b >> 7) << 6) | (b & 63); }

F110_D float beam_normal_k(uint32_t key, uint64_t step, int b) {
    float lo, hi;
    beam_normal_pair_k(key, step, beam_noise_pair(b), lo, hi);
    return (b & 64) ? hi : lo;
}

F110_D float beam_normal(uint64_t seed, uint64_t env, uint64_t step, int b) {
    return beam_normal_k(noise_key(seed, env), step, b);
}

// uniform u32 for (seed, env, episode) — autoreset spawn choice.
F110_HD uint32_t spawn_draw(uint64_t seed, uint64_t env, uint64_t episode) {
    U4 c = {(uint32_t)episode, (uint32_t)(episode >> 32), 0x5BA3Eu, 0u};
    U4 r = philox(c, (uint32_t)seed ^ (uint32_t)env, (uint32_t)(seed >> 32) ^ (uint32_t)(env >> 32) ^ 0xA5A5A5A5u);
    return r.x;
}

}  // namespace f110
