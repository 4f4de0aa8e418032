// The keyframe tables both trackers start from (tracking.hip: the IoU tracker, kalman.hip: the Kalman-filter
// tracker): a pair's detection records -> rounded KITTI label rows, compacted in row order.  One body for both
// translation units; both build with -ffp-contract=off.
#pragma once
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 128;        // rows per encoded list (max_det)
constexpr int kRecCols = 17;
constexpr int kTrk = 23;          // encoded track item: 16-col KITTI row + offsets (7)
constexpr int kK1 = 16;           // encoded keyframe-1 row
constexpr int kCnt = 4;           // [n_track_items, n_k1, skip, n_k0]

struct P2 {
    double p[12];
};

// exclusive prefix of `p` over the 256 lanes of the workgroup; *total = its sum.  Every lane calls it.
__device__ int block_scan(bool p, int* wave_tot, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(p);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int i = 0; i < kThreads / 64; ++i) {
        if (i < w) off += wave_tot[i];
        tot += wave_tot[i];
    }
    __syncthreads();
    *total = tot;
    return off + before;
}

__device__ double round3(double x) { return rint(x * 1000.0) / 1000.0; }     // np.round(x, 3)

// kitti_label_table of one record row (p: the float32 record widened, cols 0..8 = box, score, class): the rounded
// KITTI row [class, 0, 0, -10, x1, y1, x2, y2, h, w, l, x, y, z, ry, score], or false if the row does not survive.
__device__ bool kitti_row(const double* p, const P2& P, double iw, double ih, double thr, float* out) {
    if (!(p[7] >= thr)) return false;
    const double l = p[3], w = p[4], h = p[5], ry = p[6];
    const double c = cos(ry), s = sin(ry);
    double x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    for (int k = 0; k < 8; ++k) {           // project_boxes_to_image_space, the host's expression order
        const double sx = (k & 2) ? -0.5 : 0.5;
        const double sz = (k == 0 || k == 3 || k == 4 || k == 7) ? 0.5 : -0.5;
        const double xc = l * sx, zc = w * sz, yc = k < 4 ? 0.0 : -h;
        const double X = c * xc + s * zc + p[0];
        const double Y = yc + p[1];
        const double Z = -s * xc + c * zc + p[2];
        double u = P.p[0] * X + P.p[1] * Y + P.p[2] * Z + P.p[3];
        double v = P.p[4] * X + P.p[5] * Y + P.p[6] * Z + P.p[7];
        const double q = P.p[8] * X + P.p[9] * Y + P.p[10] * Z + P.p[11];
        u = u / q;
        v = v / q;
        if (k == 0) {
            x1 = x2 = u;
            y1 = y2 = v;
        } else {                            // numpy's min / max propagate NaN
            x1 = (u < x1 || isnan(u)) && !isnan(x1) ? u : x1;
            y1 = (v < y1 || isnan(v)) && !isnan(y1) ? v : y1;
            x2 = (u > x2 || isnan(u)) && !isnan(x2) ? u : x2;
            y2 = (v > y2 || isnan(v)) && !isnan(y2) ? v : y2;
        }
    }
    if (x1 > iw || y1 > ih || x2 < 0 || y2 < 0) return false;
    if (x2 - x1 > iw * 0.8 || y2 - y1 > ih * 0.8) return false;
    x1 = x1 < 0 ? 0.0 : x1;                 // np.maximum / np.minimum (NaN stays NaN)
    y1 = y1 < 0 ? 0.0 : y1;
    x2 = x2 > iw ? iw : x2;
    y2 = y2 > ih ? ih : y2;
    const double k16[16] = {0, 0, 0, -10, x1, y1, x2, y2, p[5], p[4], p[3], p[0], p[1], p[2], p[6], p[7]};
    out[0] = (float)(int32_t)p[8];
    for (int j = 1; j < 16; ++j) out[j] = (float)round3(k16[j]);
    return true;
}

// one workgroup encodes pair blockIdx.x under the calibration P and the image size iw x ih
template <typename T>
__device__ __forceinline__ void encode_pair(const T* __restrict__ records, const int32_t* __restrict__ counts,
                                            int max_det, const P2& P, double iw, double ih, double thr,
                                            float* __restrict__ trk, float* __restrict__ k1,
                                            int32_t* __restrict__ cnt) {
    __shared__ int wave_tot[kThreads / 64];
    const int pr = blockIdx.x, t = threadIdx.x;
    int n[3];
    for (int L = 0; L < 3; ++L) {           // k0, koff (keyframe 0 with the shifted box), k1
        const int slot = L == 2 ? 1 : 0;
        const int nr = min(max(counts[2 * pr + slot], 0), max_det);
        float row[16];
        bool keep = false;
        if (t < nr) {
            const T* r = records + (((size_t)pr * 2 + slot) * max_det + t) * kRecCols;
            double p[9];
            for (int c = 0; c < 9; ++c) p[c] = (double)(float)r[c];   // the host casts the records to float32 first
            if (L == 1)
                for (int c = 0; c < 7; ++c) p[c] = (double)(float)r[9 + c];
            keep = kitti_row(p, P, iw, ih, thr, row);
        }
        int tot;
        const int pos = block_scan(keep, wave_tot, &tot);
        if (keep) {
            if (L == 0) {
                float* d = trk + ((size_t)pr * kRows + pos) * kTrk;
                for (int c = 0; c < 16; ++c) d[c] = row[c];
            } else if (L == 1) {
                float* d = trk + ((size_t)pr * kRows + pos) * kTrk + 16;
                for (int c = 0; c < 7; ++c) d[c] = row[8 + c];
            } else {
                float* d = k1 + ((size_t)pr * kRows + pos) * kK1;
                for (int c = 0; c < 16; ++c) d[c] = row[c];
            }
        }
        n[L] = tot;
    }
    if (t == 0) {
        int32_t* c = cnt + (size_t)pr * kCnt;
        c[0] = min(n[0], n[1]);             // zip(k0, koff): by position, the shorter list
        c[1] = n[2];
        c[2] = n[0] == 0 && n[2] == 0;
        c[3] = n[0];
    }
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
encode_kernel(const T* __restrict__ records, const int32_t* __restrict__ counts, int max_det, P2 P, double iw,
              double ih, double thr, float* __restrict__ trk, float* __restrict__ k1, int32_t* __restrict__ cnt) {
    encode_pair(records, counts, max_det, P, iw, ih, thr, trk, k1, cnt);
}

// Lanes: pair blockIdx.x belongs to lane blockIdx.x, each lane with a calibration and an image size of its own.  The
// calibrations of a chunk of N lanes travel by value in the kernel arguments (N * 112 bytes): read before the call
// returns like p2, no upload, no lifetime; the index is blockIdx.x, uniform over the workgroup.
struct LaneCal {
    P2 P;
    double iw, ih;
};
template <int N>
struct LaneCals {
    LaneCal c[N];
};
__device__ bool lane_on(unsigned mask, int lane) { return (mask >> lane) & 1u; }

template <typename T, int N>
__global__ void __launch_bounds__(kThreads)
encode_lanes_kernel(const T* __restrict__ records, const int32_t* __restrict__ counts, int max_det, LaneCals<N> tab,
                    unsigned mask, double thr, float* __restrict__ trk, float* __restrict__ k1,
                    int32_t* __restrict__ cnt) {
    if (!lane_on(mask, blockIdx.x)) return;
    const LaneCal& cal = tab.c[blockIdx.x];
    encode_pair(records, counts, max_det, cal.P, cal.iw, cal.ih, thr, trk, k1, cnt);
}

}  // namespace
