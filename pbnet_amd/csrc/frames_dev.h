// frames_dev.h -- the validity test of a depth sample, shared by frames.hip (back-projection) and tsdf.hip (fusion): rules
// (b) and (c) of include/pbnet_hip.h's "Posed depth frames".  Float64 comparisons and one product; every translation unit
// that includes it is built with -ffp-contract=off.
#pragma once
#include "pbn_common.h"

namespace pbn {
namespace {

__device__ __forceinline__ double frames_z(unsigned short d, double scale) { return (double)d / scale; }
__device__ __forceinline__ double frames_z(float d, double) { return (double)d; }

// rule (b); a uint16 0 gives z = 0 and fails z > 0
__device__ __forceinline__ bool frames_measured(double z, double z_min, double z_max) {
    return __builtin_isfinite(z) && z > 0.0 && z >= z_min && z <= z_max;
}

// Pixel (u, v) of one frame's image `img` [height, width]: z, and whether it is measured (b) and -- with edge > 0 -- no
// measured 4-neighbour inside the image differs from it by more than edge * z (c).
template <typename D>
__device__ __forceinline__ bool frames_depth_ok(const D* __restrict__ img, int height, int width, int u, int v, double scale,
                                                double z_min, double z_max, double edge, double& z) {
    z = frames_z(img[(size_t)v * width + u], scale);
    if (!frames_measured(z, z_min, z_max)) return false;
    if (edge > 0.0) {
        const double lim = edge * z;
        bool is_edge = false;
        if (u > 0) {
            const double zn = frames_z(img[(size_t)v * width + (u - 1)], scale);
            is_edge |= frames_measured(zn, z_min, z_max) && fabs(zn - z) > lim;
        }
        if (u + 1 < width) {
            const double zn = frames_z(img[(size_t)v * width + (u + 1)], scale);
            is_edge |= frames_measured(zn, z_min, z_max) && fabs(zn - z) > lim;
        }
        if (v > 0) {
            const double zn = frames_z(img[(size_t)(v - 1) * width + u], scale);
            is_edge |= frames_measured(zn, z_min, z_max) && fabs(zn - z) > lim;
        }
        if (v + 1 < height) {
            const double zn = frames_z(img[(size_t)(v + 1) * width + u], scale);
            is_edge |= frames_measured(zn, z_min, z_max) && fabs(zn - z) > lim;
        }
        if (is_edge) return false;
    }
    return true;
}

// rule (a): the 12 numbers of the top three rows
__device__ __forceinline__ bool frames_pose_ok(const double* __restrict__ P) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && __builtin_isfinite(P[i]);
    return ok;
}

}  // namespace
}  // namespace pbn
