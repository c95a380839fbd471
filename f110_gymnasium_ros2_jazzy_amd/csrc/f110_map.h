// f110_map.h — the EDT map as the kernels see it: the row-major and the tiled view and the cell
// index of a lookup at (x, y) (xy_2_rc + distance_transform).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f110_math.h"

namespace f110 {

// -------------------------------------------------------------- the map --
struct MapView {
    const double *dt;  // [H*W] metres (res * EDT), row-major
    int32_t H, W;
    int64_t n;         // H*W
    double res, ox, oy, oc, os;
    double wres, hres; // width*resolution, height*resolution (laser_models.py:79)
    double inv_res;    // fl(1 / res), for the guarded fast quotient below
};

// xy_2_rc + distance_transform, laser_models.py:55-104: the linear EDT index
// a lookup at (x, y) reads.  Out-of-map (r,c) = (-1,-1) reads dt[-1,-1].
F110_HD int64_t cell_index(const MapView &m, double x, double y) {
    double xt = x - m.ox;
    double yt = y - m.oy;
    double xr = xt * m.oc + yt * m.os;
    double yr = -xt * m.os + yt * m.oc;
    if (xr < 0 || xr >= m.wres || yr < 0 || yr >= m.hres || xr != xr || yr != yr) return m.n - 1;
    int c = (int)(xr / m.res);
    int r = (int)(yr / m.res);
    int64_t lin = (int64_t)r * m.W + c;
    return lin < m.n ? lin : m.n - 1;
}

// int(v / res) for 0 <= v < W*res without the fp64 divide on the common
// path.  fl(v * fl(1/res)) and fl(v / res) are both within 2^-52 relative of
// the exact quotient (< 1e-12 absolute for v/res < 4096), so their integer
// parts agree unless the quotient lies within that distance of an integer;
// inside a 1e-9 guard band the IEEE division decides (bit-exact with
// xy_2_rc's int(x_rot/resolution), laser_models.py:83-84).
F110_HD int trunc_div(double v, double res, double inv_res) {
    double q = v * inv_res;
    int k = (int)q;
    double f = q - (double)k;
    if (f < 1e-9 || f > 1.0 - 1e-9) k = (int)(v / res);
    return k;
}

F110_HD int64_t cell_index_fast(const MapView &m, double x, double y) {
    double xt = x - m.ox;
    double yt = y - m.oy;
    double xr = xt * m.oc + yt * m.os;
    double yr = -xt * m.os + yt * m.oc;
    if (xr < 0 || xr >= m.wres || yr < 0 || yr >= m.hres || xr != xr || yr != yr) return m.n - 1;
    int c = trunc_div(xr, m.res, m.inv_res);
    int r = trunc_div(yr, m.res, m.inv_res);
    int64_t lin = (int64_t)r * m.W + c;
    return lin < m.n ? lin : m.n - 1;
}

// The EDT in 4x4-cell tiles (16 f64 = one 128-B cache line): the 64 lanes of
// a wave trace 64 neighbouring beams whose samples form a short arc of cells
// in ANY direction; square tiles bound the cache lines that arc touches,
// where row-major lines are 16 x 1 cells and an arc along a column touches
// one line per cell.
struct TiledMapView {
    const double *dt;  // [(Hp/4)*(Wp/4)][16], Hp/Wp = H/W rounded up to 4
    int32_t H, W, wt;  // wt = Wp / 4 tiles per tile-row
    int32_t oob;       // tiled index of dt[H-1][W-1] (the reference's dt[-1,-1])
    double res, inv_res, ox, oy, oc, os, wres, hres;
};

// Cells are column-major inside a tile: index = tile * 16 + (c & 3) * 4 +
// (r & 3), so (c >> 2) * 16 + (c & 3) * 4 == c * 4 and the index is
// (r >> 2) * wt * 16 + c * 4 + (r & 3) -- one multiply-add (k_rays_fx).
F110_HD int32_t tiled_index(int32_t wt, int32_t r, int32_t c) {
    return (r >> 2) * wt * 16 + c * 4 + (r & 3);
}

// xy_2_rc + distance_transform (laser_models.py:55-104) on the tiled EDT.
// ROT = false when the map's origin yaw is exactly 0 (cos = 1, sin = 0): then
// x_rot = x_trans*1 + y_trans*0 == x_trans for every finite input (a NaN or
// inf input still lands off-map), so the rotation is skipped bit-exactly.
template <bool ROT>
F110_HD int32_t tiled_cell(const TiledMapView &m, double x, double y) {
    double xr = x - m.ox;
    double yr = y - m.oy;
    if (ROT) {
        const double xt = xr, yt = yr;
        xr = xt * m.oc + yt * m.os;
        yr = -xt * m.os + yt * m.oc;
    }
    const bool inb = (xr >= 0) & (xr < m.wres) & (yr >= 0) & (yr < m.hres);  // false for NaN
    const double qx = xr * m.inv_res, qy = yr * m.inv_res;
#if defined(__HIP_DEVICE_COMPILE__)
    const double fx = __builtin_amdgcn_fract(qx), fy = __builtin_amdgcn_fract(qy);
#else
    const double fx = qx - floor(qx), fy = qy - floor(qy);
#endif
    // the conversions see in-range values only (a NaN or out-of-range double -> int is UB;
    // off-map results are discarded below)
    int32_t c = (int32_t)(inb ? qx : 0.0), r = (int32_t)(inb ? qy : 0.0);
    // guard band (see trunc_div): near an integer the IEEE quotient decides
    const double band = fmax(fabs(fx - 0.5), fabs(fy - 0.5));
    if (inb && band > 0.5 - 1e-9) {
        c = (int32_t)(xr / m.res);
        r = (int32_t)(yr / m.res);
        // x_rot < W*res and y_rot < H*res, yet the rounded quotient can reach W
        // (or H) exactly.  Same cell as cell_index's flat row-major read:
        // dt[r, W] is dt[r+1, 0]; anything past the last cell is dt[-1, -1].
        if (c >= m.W) {
            c = 0;
            ++r;
        }
        if (r >= m.H) return m.oob;
    }
    return inb ? tiled_index(m.wt, r, c) : m.oob;
}

// The ray loop's form of tiled_cell (same cell, bit for bit): the tile index
// in 24-bit multiplies, the IEEE-divide fallback behind a wave-uniform
// branch (taken only when some lane sits within 1e-9 of a cell edge, so the
// common iteration carries no exec-mask juggling), and the EDT read as a
// 32-bit byte offset from the table base (SGPR-base global load).
__device__ __forceinline__ uint32_t tiled_index_u24(int32_t wt, int32_t r, int32_t c) {
    return __umul24((uint32_t)r >> 2, (uint32_t)wt << 4) + (((uint32_t)c << 2) | ((uint32_t)r & 3u));
}

// the same cell as a byte offset into the f64 table
__device__ __forceinline__ uint32_t tiled_offset_u24(int32_t wt, int32_t r, int32_t c) {
    return (__umul24((uint32_t)r >> 2, (uint32_t)wt) << 7) + (((uint32_t)c << 5) | (((uint32_t)r & 3u) << 3));
}

// oob8: the byte offset of m.oob (m.oob << 3), passed by the caller so that a
// loop can keep it in a VGPR (the select below cannot read it from an SGPR
// next to its VCC condition)
template <bool ROT>
__device__ __forceinline__ double tiled_lookup(const TiledMapView &m, double x, double y, uint32_t oob8) {
    double xr = x - m.ox;
    double yr = y - m.oy;
    if (ROT) {
        const double xt = xr, yt = yr;
        xr = xt * m.oc + yt * m.os;
        yr = -xt * m.os + yt * m.oc;
    }
    const bool inb = (xr >= 0) & (xr < m.wres) & (yr >= 0) & (yr < m.hres);  // false for NaN
    const double qx = xr * m.inv_res, qy = yr * m.inv_res;
#if defined(__HIP_DEVICE_COMPILE__)
    const double fx = __builtin_amdgcn_fract(qx), fy = __builtin_amdgcn_fract(qy);
#else
    const double fx = qx - floor(qx), fy = qy - floor(qy);
#endif
    const double band = fmax(fabs(fx - 0.5), fabs(fy - 0.5));
    const bool near = band > 0.5 - 1e-9;  // the guard band of trunc_div (off-map lanes filtered inside)
    // off-map lanes convert 0 (a NaN or out-of-range double -> int is UB); their offset is masked below
    const uint32_t fast = tiled_offset_u24(m.wt, (int32_t)(inb ? qy : 0.0), (int32_t)(inb ? qx : 0.0));
    const uint32_t sel = 0u - (uint32_t)inb;  // branchless select: no exec-mask split per iteration
    uint32_t off = (fast & sel) | (oob8 & ~sel);
#if defined(__HIP_DEVICE_COMPILE__)
    // wave-uniform, rare; the ballot of a bare compare is its lane mask (no
    // VGPR round trip, as a ballot of (inb && near) would need)
    if (__builtin_amdgcn_ballot_w64(near))
#endif
    {
        if (near && inb) {
            int32_t c = (int32_t)(xr / m.res);
            int32_t r = (int32_t)(yr / m.res);
            if (c >= m.W) {  // see tiled_cell
                c = 0;
                ++r;
            }
            off = r >= m.H ? oob8 : tiled_offset_u24(m.wt, r, c);
        }
    }
    return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(m.dt) + off);
}

}  // namespace f110
