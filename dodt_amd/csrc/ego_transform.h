// The ego-motion half of cal_transformed_ious, shared by the Kalman-filter tracker (kalman.hip) and the velocity tracker
// (velocity_track.hip): a detection's box moved into the frame of the keyframe before it (label_transform_box on the
// host: corners -> velo -> (+trans) @ matrix -> rect, the host's expression order).  One body for both translation
// units; both build with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace {

struct KfCalib {            // ops.temporal_calib: inv(R0_rect), inv(Tr_velo_to_cam) (3x4), Tr_velo_to_cam, R0_rect
    double r0_inv[9], tr_inv[12], tr[12], r0[9];
};

// det [h,w,l,x,y,z,ry] under the ego row `ego` (trans (3), matrix (3x3, row major), delta) -> b [x,y,z,l,w,h,ry], the
// moved box in iou_3d's order
__device__ void ego_moved_box(const double* det, const double* ego, const KfCalib& k, double* b) {
    const double h = det[0], w = det[1], l = det[2], x = det[3], y = det[4], z = det[5], ry = det[6];
    const double c = cos(ry), s = sin(ry);
    const double rot[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    const double xc[8] = {l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2};
    const double yc[8] = {0, 0, 0, 0, -h, -h, -h, -h};
    const double zc[8] = {w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2};
    const double org[3] = {x, y, z};
    double sum[3] = {0, 0, 0};
    for (int v = 0; v < 8; ++v) {
        double p[3], ref[3], velo[3], v2[3], ref2[3];
        for (int r = 0; r < 3; ++r)
            p[r] = rot[3 * r] * xc[v] + rot[3 * r + 1] * yc[v] + rot[3 * r + 2] * zc[v] + org[r];
        for (int r = 0; r < 3; ++r)
            ref[r] = k.r0_inv[3 * r] * p[0] + k.r0_inv[3 * r + 1] * p[1] + k.r0_inv[3 * r + 2] * p[2];
        for (int r = 0; r < 3; ++r)
            velo[r] = ref[0] * k.tr_inv[4 * r] + ref[1] * k.tr_inv[4 * r + 1] + ref[2] * k.tr_inv[4 * r + 2]
                      + k.tr_inv[4 * r + 3];
        for (int r = 0; r < 3; ++r)
            v2[r] = (velo[0] + ego[0]) * ego[3 + r] + (velo[1] + ego[1]) * ego[6 + r] + (velo[2] + ego[2]) * ego[9 + r];
        for (int r = 0; r < 3; ++r)
            ref2[r] = v2[0] * k.tr[4 * r] + v2[1] * k.tr[4 * r + 1] + v2[2] * k.tr[4 * r + 2] + k.tr[4 * r + 3];
        for (int r = 0; r < 3; ++r)
            sum[r] += k.r0[3 * r] * ref2[0] + k.r0[3 * r + 1] * ref2[1] + k.r0[3 * r + 2] * ref2[2];
    }
    b[0] = sum[0] / 8;
    b[1] = sum[1] / 8 + h / 2.0;
    b[2] = sum[2] / 8;
    b[3] = l;
    b[4] = w;
    b[5] = h;
    b[6] = ry + ego[12];
}

}  // namespace
