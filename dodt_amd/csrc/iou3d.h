// The 3-D IoU of two [x,y,z,l,w,h,ry] boxes in float64, shared by the temporal module (temporal.hip) and the tracker
// (tracking.hip): dt_evaluator_utils.three_d_iou_matrix expression by expression.  Both translation units build with
// -ffp-contract=off, so every product and sum stays unfused and the two give the same bits for the same boxes.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int kVerts = 12;        // a convex polygon clipped by four half-planes has at most 8 vertices

// three_d_iou_matrix (dt_evaluator_utils.py) of one pair of [x,y,z,l,w,h,ry] boxes
__device__ double iou_3d(const double* a, const double* b) {
    const double diag_a = sqrt(a[3] * a[3] + a[4] * a[4] + a[5] * a[5]) / 2;
    const double diag_b = sqrt(b[3] * b[3] + b[4] * b[4] + b[5] * b[5]) / 2;
    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    const double dist = sqrt(dx * dx + dy * dy + dz * dz);
    if (!(diag_a + diag_b >= dist)) return 0.0;
    const double h_int = fmax(0.0, fmin(a[1], b[1]) - fmax(a[1] - a[5], b[1] - b[5]));
    // _rects: base corners (x, z)
    double px[kVerts], pz[kVerts], qx[4], qz[4];
    {
        const double c = cos(a[6]), s = sin(a[6]), hl = a[3] / 2, hw = a[4] / 2;
        const double xc[4] = {hl, hl, -hl, -hl}, zc[4] = {hw, -hw, -hw, hw};
        for (int k = 0; k < 4; ++k) {
            px[k] = c * xc[k] + s * zc[k] + a[0];
            pz[k] = -s * xc[k] + c * zc[k] + a[2];
        }
    }
    {
        const double c = cos(b[6]), s = sin(b[6]), hl = b[3] / 2, hw = b[4] / 2;
        const double xc[4] = {hl, hl, -hl, -hl}, zc[4] = {hw, -hw, -hw, hw};
        for (int k = 0; k < 4; ++k) {
            qx[k] = c * xc[k] + s * zc[k] + b[0];
            qz[k] = -s * xc[k] + c * zc[k] + b[2];
        }
    }
    // base_intersections: the clip polygon counter-clockwise
    const double e0x = qx[1] - qx[0], e0z = qz[1] - qz[0], e1x = qx[2] - qx[1], e1z = qz[2] - qz[1];
    if (e0x * e1z - e0z * e1x < 0) {
        double t;
        t = qx[0]; qx[0] = qx[3]; qx[3] = t; t = qx[1]; qx[1] = qx[2]; qx[2] = t;
        t = qz[0]; qz[0] = qz[3]; qz[3] = t; t = qz[1]; qz[1] = qz[2]; qz[2] = t;
    }
    int cnt = 4;
    for (int e = 0; e < 4; ++e) {       // _clip_batch against edge q[e] -> q[e + 1]
        const double ax = qx[e], az = qz[e];
        const double d0 = qx[(e + 1) & 3] - ax, d1 = qz[(e + 1) & 3] - az;
        double side[kVerts], nx[kVerts], nz[kVerts];
        for (int v = 0; v < cnt; ++v) side[v] = d0 * (pz[v] - az) - d1 * (px[v] - ax);
        int m = 0;
        for (int v = 0; v < cnt; ++v) {
            const int j = v + 1 < cnt ? v + 1 : 0;
            const bool in_v = side[v] >= 0, in_j = side[j] >= 0;
            if (in_v && m < kVerts) {
                nx[m] = px[v];
                nz[m] = pz[v];
                ++m;
            }
            if (in_v != in_j && m < kVerts) {
                const double t = side[v] / (side[v] - side[j]);
                nx[m] = px[v] + t * (px[j] - px[v]);
                nz[m] = pz[v] + t * (pz[j] - pz[v]);
                ++m;
            }
        }
        for (int v = 0; v < m; ++v) {
            px[v] = nx[v];
            pz[v] = nz[v];
        }
        cnt = m;
    }
    // shoelace over eight slots, the ones behind the polygon repeating vertex 0; numpy's pairwise sum of eight terms
    double sx[8], sz[8];
    for (int v = 0; v < 8; ++v) {
        const int u = v < cnt ? v : 0;
        sx[v] = px[u];
        sz[v] = pz[u];
    }
    double t1[8], t2[8];
    for (int v = 0; v < 8; ++v) {
        t1[v] = sx[v] * sz[(v + 1) & 7];
        t2[v] = sz[v] * sx[(v + 1) & 7];
    }
    const double s1 = ((t1[0] + t1[1]) + (t1[2] + t1[3])) + ((t1[4] + t1[5]) + (t1[6] + t1[7]));
    const double s2 = ((t2[0] + t2[1]) + (t2[2] + t2[3])) + ((t2[4] + t2[5]) + (t2[6] + t2[7]));
    const double area = cnt >= 3 ? 0.5 * fabs(s1 - s2) : 0.0;     // (and 0 / 0 stays NaN, as on the host)
    const double inter = h_int * area;
    return inter / (a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - inter);
}

}  // namespace
