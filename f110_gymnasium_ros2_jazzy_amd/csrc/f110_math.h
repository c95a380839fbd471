// f110_math.h — the bottom of the include graph of the device (and host/device) building blocks:
// the F110_HD / F110_D function macros, the constants and the scalar helpers (np.clip, Python's
// float remainder, the yaw wrap).
//
// Semantics restate the reference hot path term by term (paths relative to
// f110_gymnasium/gym/f110_gym/envs/ of ahoop004/f110_gymnasium_ros2_jazzy).
// Compiled with -ffp-contract=off: every a*b+c below rounds twice, exactly as
// the Python/Numba source does.  Where the reference's NumPy calls reach BLAS
// (ndarray.dot, np.linalg.norm) the rounding pattern of the reference run is
// reproduced with explicit fma() (see DESIGN.md "Rounding contract").
#pragma once

#include <hip/hip_runtime.h>

#define F110_HD __host__ __device__ __forceinline__
#define F110_D __device__ __forceinline__

namespace f110 {

constexpr double kPi = 3.141592653589793;      // np.pi
constexpr double kTwoPi = 6.283185307179586;   // 2 * np.pi
constexpr double kHalfPi = 1.5707963267948966; // np.pi / 2
constexpr double kSlipCap = 1.0471975511965976; // np.deg2rad(60)  (base_classes.py:414)
constexpr double kYawRateCap = 10.0;           // base_classes.py:410
constexpr double kG = 9.81;                    // dynamic_models.py:146
constexpr int kMaxAgents = 8;
constexpr int kMaxSeg = 80;

// ----------------------------------------------------------------- scalars --
F110_HD double clip(double a, double lo, double hi) {  // np.clip (NaN propagates)
    if (a != a) return a;
    return a < lo ? lo : (a > hi ? hi : a);
}

// Python / NumPy float remainder (npy_divmod): result takes the divisor's sign.
F110_HD double pymod(double a, double b) {
    double mod = fmod(a, b);
    if (mod != 0.0) {
        if ((b < 0) != (mod < 0)) mod += b;
    } else {
        mod = copysign(0.0, b);
    }
    return mod;
}

// pymod for 0 <= a < b (the yaw wraps' common case): a itself, +0 for a zero of either sign --
// what fmod and the sign fix-up give there -- without the library's fmod loop.
F110_HD double pymod_fast(double a, double b) {
    if (b > 0.0 && a >= 0.0 && a < b) return a == 0.0 ? 0.0 : a;
    return pymod(a, b);
}

// F110Env._wrap_angle / update_pose yaw wrap: ((a + pi) % 2pi) - pi.
F110_HD double wrap_angle(double a) { return pymod_fast(a + kPi, kTwoPi) - kPi; }

}  // namespace f110
