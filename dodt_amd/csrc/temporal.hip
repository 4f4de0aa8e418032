// Temporal module "M" of S+T+M on the device (dodt_amd/core/dt_evaluator_utils.py, which mirrors the reference's
// avod/core/dt_evaluator_utils.py:212-362): associate the detections of a keyframe pair by 3-D IoU and fill in the
// frames between them.
//
// Float64 throughout, the host module's arithmetic expression by expression (the Makefile's -ffp-contract=off keeps
// every product and sum unfused): the records are widened to double first, the IoU is three_d_iou_matrix (bounding-
// sphere early exit, height overlap, Sutherland-Hodgman clipping of the two bases against the counter-clockwise
// clip rectangle, shoelace area summed in numpy's pairwise order over the eight vertex slots), the interpolation is
// interpolate_non_keyframe_predictions + _fill case by case.  cos/sin come from the device's math library, so a
// result may differ from the host's in its last bits.
//
// Two launches.  pair_iou_kernel: the IoU of every row pair that passes the threshold, one lane each over the whole
// chip, into a per-context workspace.  interpolate_kernel: one workgroup (256 lanes, four waves) per pair.  LDS: the
// kept k0 x k1 IoU matrix gathered from the workspace (doubles; 100 x 100 = 80 000 bytes, at most 128 x 128 =
// 128 KiB), dynamic; the small index tables static.  The row argmaxes of the greedy match do not depend on which columns are still free, so
// they are computed one lane per row; only the walk over the rows with the free mask is sequential (wave 0).
// Output rows are placed by a workgroup prefix over the items (matched and unmatched keyframe-0 detections in
// order, then the free keyframe-1 detections in index order), one prefix per frame.
// The recovery's calibration is the launch's one, a kernel argument, or one row per pair of a device array
// (dodt_interpolate_pairs_calibs): the same kernel body, instantiated for either.
#include "common.h"
#include "iou3d.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDet = 128;      // items (<= 2 * max_det) must fit the 256 lanes; the matrix the LDS
constexpr int kRecCols = 17;
constexpr int kOutCols = 13;
constexpr int kMaxFrames = 64;

struct Calib {                    // kitti_tracking_utils._rect_to_velo / _velo_to_rect
    double r0_inv[9], tr_inv[12], tr[12], r0[9];
};

__global__ void __launch_bounds__(256)
iou_matrix_kernel(const double* __restrict__ a, int na, const double* __restrict__ b, int nb, double* __restrict__ out) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long long)na * nb) return;
    const int i = (int)(q / nb), j = (int)(q % nb);
    double ba[7], bb[7];
    for (int c = 0; c < 7; ++c) {
        ba[c] = a[(size_t)i * 7 + c];
        bb[c] = b[(size_t)j * 7 + c];
    }
    out[q] = iou_3d(ba, bb);
}

// kitti_tracking_utils.recovery_coordinate of one row: corners -> velo -> undo (trans, matrix) -> rect, their mean,
// + h/2 on y; ry - delta.  ego: [trans(3), inv(matrix) (3x3 row-major), delta].
__device__ void recover_row(double* row, const double* ego, const Calib& k) {
    const double x = row[0], y = row[1], z = row[2], l = row[3], w = row[4], h = row[5], ry = row[6];
    const double c = cos(ry), s = sin(ry);
    const double rot[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    const double xc[8] = {l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2};
    const double yc[8] = {0, 0, 0, 0, -h, -h, -h, -h};
    const double zc[8] = {w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2};
    double sum[3] = {0, 0, 0};
    for (int v = 0; v < 8; ++v) {
        double p[3];
        const double org[3] = {x, y, z};
        for (int r = 0; r < 3; ++r)
            p[r] = rot[3 * r] * xc[v] + rot[3 * r + 1] * yc[v] + rot[3 * r + 2] * zc[v] + org[r];
        double ref[3], velo[3], v2[3], ref2[3];
        for (int r = 0; r < 3; ++r)
            ref[r] = k.r0_inv[3 * r] * p[0] + k.r0_inv[3 * r + 1] * p[1] + k.r0_inv[3 * r + 2] * p[2];
        for (int r = 0; r < 3; ++r)
            velo[r] = ref[0] * k.tr_inv[4 * r] + ref[1] * k.tr_inv[4 * r + 1] + ref[2] * k.tr_inv[4 * r + 2]
                      + k.tr_inv[4 * r + 3];
        for (int r = 0; r < 3; ++r)
            v2[r] = velo[0] * ego[3 + r] + velo[1] * ego[6 + r] + velo[2] * ego[9 + r] - ego[r];
        for (int r = 0; r < 3; ++r)
            ref2[r] = v2[0] * k.tr[4 * r] + v2[1] * k.tr[4 * r + 1] + v2[2] * k.tr[4 * r + 2] + k.tr[4 * r + 3];
        for (int r = 0; r < 3; ++r)
            sum[r] += k.r0[3 * r] * ref2[0] + k.r0[3 * r + 1] * ref2[1] + k.r0[3 * r + 2] * ref2[2];
    }
    row[0] = sum[0] / 8;
    row[1] = sum[1] / 8 + h / 2.0;
    row[2] = sum[2] / 8;
    row[6] = ry - ego[12];
}

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

template <typename T>
__device__ void load_row(const T* rec, double* row) {
    for (int c = 0; c < kRecCols; ++c) row[c] = (double)rec[c];
}

// The IoU of every row pair of a keyframe pair whose scores both pass the threshold, spread over the whole chip: one lane
// per (pair, row of keyframe 0, row of keyframe 1) into ws (n_pairs, max_det, max_det), which interpolate_kernel then
// gathers for its kept rows (in one workgroup per pair these clipped fp64 IoUs took half a millisecond per pair).
template <typename T>
__global__ void __launch_bounds__(256)
pair_iou_kernel(const T* __restrict__ records, const int32_t* __restrict__ counts, int max_det, double threshold,
                double* __restrict__ ws) {
    const int p = blockIdx.y;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= max_det * max_det) return;
    const int i = q / max_det, j = q % max_det;
    const int n0 = min(max(counts[2 * p], 0), max_det), n1 = min(max(counts[2 * p + 1], 0), max_det);
    if (i >= n0 || j >= n1) return;
    const T* ra = records + ((size_t)p * 2 * max_det + i) * kRecCols;
    const T* rb = records + ((size_t)p * 2 * max_det + max_det + j) * kRecCols;
    if (!((double)ra[7] > threshold && (double)rb[7] > threshold)) return;
    double ba[7], bb[7];
    for (int c = 0; c < 7; ++c) {
        ba[c] = (double)ra[c];
        bb[c] = (double)rb[c];
    }
    ws[(size_t)p * max_det * max_det + q] = iou_3d(ba, bb);
}

// The calibration pair p recovers with: the launch's one (by value, dodt_interpolate_pairs) or row p of a device array
// (dodt_interpolate_pairs_calibs: the address is the same for every lane of the workgroup, so the 42 doubles come
// through the scalar cache and cost neither vector registers nor LDS).
__device__ inline const Calib& calib_of_pair(const Calib& one, int) { return one; }
__device__ inline const Calib& calib_of_pair(const Calib* rows, int p) { return rows[p]; }

template <typename T, typename CalibArg>
__global__ void __launch_bounds__(kThreads)
interpolate_kernel(const T* __restrict__ records, const int32_t* __restrict__ counts, int max_det, int nf,
                   double threshold, int next_best, const double* __restrict__ recover, CalibArg calib_arg, int max_out,
                   const double* __restrict__ ws, double* __restrict__ out, int32_t* __restrict__ out_counts,
                   int32_t* __restrict__ status) {
    extern __shared__ double lds[];
    __shared__ int kept[2][kMaxDet], best[kMaxDet], match[kMaxDet], freelist[kMaxDet];
    __shared__ int wave_tot[kThreads / 64], s_k[2], s_nfree, s_status;
    const int p = blockIdx.x, t = threadIdx.x;
    const Calib& calib = calib_of_pair(calib_arg, p);
    const bool assoc = nf >= 3;
    double* M = lds;                                          // k0 x k1, row stride k1 (association only)
    const T* rec = records + (size_t)p * 2 * max_det * kRecCols;
    double* o = out + (size_t)p * nf * max_out * kOutCols;
    const double* ego = recover ? recover + (size_t)p * nf * 13 : nullptr;

    // keyframe rows with score > threshold (the score widened first), in order
    const int nk = nf >= 2 ? 2 : 1;
    for (int f = 0; f < nk; ++f) {
        const int n = min(max(counts[2 * p + f], 0), max_det);
        const T* r = rec + ((size_t)f * max_det + t) * kRecCols;
        const bool keep = t < n && (double)r[7] > threshold;
        int tot;
        const int pos = block_scan(keep, wave_tot, &tot);
        if (keep) kept[f][pos] = t;
        if (t == 0) s_k[f] = tot;
    }
    __syncthreads();
    const int k0 = s_k[0], k1 = nk == 2 ? s_k[1] : 0;

    if (!assoc) {         // n_frames 1 and 2: keyframe 0 as it is, keyframe 1 recovered
        for (int f = 0; f < nk; ++f) {
            const int kf = f == 0 ? k0 : k1;
            for (int i = t; i < kf; i += kThreads) {
                double row[kRecCols];
                load_row(rec + ((size_t)f * max_det + kept[f][i]) * kRecCols, row);
                if (f == 1 && ego) recover_row(row, ego + 13, calib);
                double* dst = o + ((size_t)f * max_out + i) * kOutCols;
                for (int c = 0; c < kOutCols; ++c) dst[c] = row[c];
            }
            if (t == 0) out_counts[p * nf + f] = kf;
        }
        if (t == 0) status[p] = 0;
        return;
    }

    // IoU of every kept keyframe-0 detection with every kept keyframe-1 detection (pair_iou_kernel's)
    const double* w = ws + (size_t)p * max_det * max_det;
    for (int q = t; q < k0 * k1; q += kThreads) M[q] = w[(size_t)kept[0][q / k1] * max_det + kept[1][q % k1]];
    __syncthreads();
    // row argmax over all columns, first index on ties (np.argmax)
    if (t < k0 && k1 > 0) {
        const double* row = M + (size_t)t * k1;
        int bi = 0;
        double bv = row[0];
        for (int j = 1; j < k1; ++j)
            if (row[j] > bv) {
                bv = row[j];
                bi = j;
            }
        best[t] = bi;
    }
    __syncthreads();
    // the greedy walk with the free mask: wave 0, row by row (a still-free best match is the common case; the argmax
    // over the free columns that a taken one needs in 'next_best' mode is a wave reduction)
    if (t < 64) {
        unsigned long long fm[2] = {0ull, 0ull};
        for (int j = 0; j < k1; ++j) fm[j >> 6] |= 1ull << (j & 63);
        int nfree = k1, st = 0;
        for (int n = 0; n < k0; ++n) {
            int m = -1;
            if (nfree > 0) {
                const double* row = M + (size_t)n * k1;
                int b = best[n];
                double v = row[b];
                if (v > 0 && !((fm[b >> 6] >> (b & 63)) & 1ull)) {
                    if (!next_best) {       // the reference's next_idx.remove raises
                        st = 1;
                        break;
                    }
                    // argmax over the still-free columns, first index on ties
                    double bv = -INFINITY;
                    int bi = INT_MAX;
                    for (int j = t; j < k1; j += 64)
                        if (((fm[j >> 6] >> (j & 63)) & 1ull) && (bi == INT_MAX || row[j] > bv)) {
                            bv = row[j];
                            bi = j;
                        }
                    for (int off = 32; off > 0; off >>= 1) {
                        const double ov = __shfl_xor(bv, off);
                        const int oi = __shfl_xor(bi, off);
                        if (ov > bv || (ov == bv && oi < bi)) {
                            bv = ov;
                            bi = oi;
                        }
                    }
                    b = bi;
                    v = bv;
                }
                if (v > 0) {
                    m = b;
                    fm[b >> 6] &= ~(1ull << (b & 63));
                    --nfree;
                }
            }
            if (t == 0) match[n] = m;
        }
        if (t == 0) {
            int c = 0;
            for (int j = 0; j < k1; ++j)
                if ((fm[j >> 6] >> (j & 63)) & 1ull) freelist[c++] = j;
            s_nfree = nfree;
            s_status = st;
        }
    }
    __syncthreads();
    if (s_status) {
        for (int f = t; f < nf; f += kThreads) out_counts[p * nf + f] = 0;
        if (t == 0) status[p] = s_status;
        return;
    }

    // items: keyframe-0 detections (matched or not), then the free keyframe-1 detections; lane t holds item t
    const int n_items = k0 + s_nfree;
    const bool valid = t < n_items;
    int ia = -1, ib = -1;
    if (valid) {
        if (t < k0) {
            ia = t;
            ib = match[t];
        } else {
            ib = freelist[t - k0];
        }
    }
    double ra[kRecCols], rb[kRecCols];
    if (ia >= 0) load_row(rec + (size_t)kept[0][ia] * kRecCols, ra);
    if (ib >= 0) load_row(rec + ((size_t)max_det + kept[1][ib]) * kRecCols, rb);
    const bool both = ia >= 0 && ib >= 0, first = ia >= 0;
    const double* only = first ? ra : rb;
    double score = 0, d = 0, dx = 0, dz = 0;
    bool near = false;
    if (valid && both) {
        score = rb[7] > ra[7] ? rb[7] : ra[7];
    } else if (valid) {         // _fill: offsets = only[-4:-1]
        d = sqrt(only[13] * only[13] + only[14] * only[14]);
        near = d <= only[4] / 2;
        dx = d * cos(only[6]);
        dz = d * sin(only[6]);
    }
    const double num = (double)nf, den = (double)(nf - 1);
    for (int f = 0; f < nf; ++f) {
        double row[kOutCols];
        bool present = valid;
        if (valid && both) {
            if (f == 0) {
                for (int c = 0; c < kOutCols; ++c) row[c] = ra[c];
            } else if (f == nf - 1) {
                for (int c = 0; c < kOutCols; ++c) row[c] = rb[c];
                row[7] = score;
            } else {
                const double i1 = (double)(f - 1) + 1.0;
                for (int c = 0; c < kOutCols; ++c) row[c] = ra[c];
                row[0] = ra[0] + (rb[0] - ra[0]) * i1 / den;
                row[2] = ra[2] + (rb[2] - ra[2]) * i1 / den;
                row[6] = ra[6] + (rb[6] - ra[6]) * i1 / den;
                row[7] = score;
            }
        } else if (valid && first) {        // seen in keyframe 0 only: moves on, or dies after half of the frames
            for (int c = 0; c < kOutCols; ++c) row[c] = ra[c];
            if (f > 0) {
                const int i = f - 1;
                if (near) {
                    row[0] = ra[0] + dx * ((double)i + 1.0) / den;
                    row[2] = ra[2] + dz * ((double)i + 1.0) / den;
                } else {
                    present = !((double)i >= num / 2);
                }
            }
        } else if (valid) {                 // seen in keyframe 1 only: traced back, or born after half of the frames
            for (int c = 0; c < kOutCols; ++c) row[c] = rb[c];
            if (f < nf - 1) {
                const int i = f;
                if (near) {
                    row[0] = rb[0] - dx * (double)(nf - i - 2) / den;
                    row[2] = rb[2] - dz * (double)(nf - i - 2) / den;
                } else {
                    present = !((double)i <= num / 2);
                }
            }
        }
        int tot;
        const int pos = block_scan(present, wave_tot, &tot);
        if (present) {
            if (f > 0 && ego) recover_row(row, ego + (size_t)f * 13, calib);
            double* dst = o + ((size_t)f * max_out + pos) * kOutCols;
            for (int c = 0; c < kOutCols; ++c) dst[c] = row[c];
        }
        if (t == 0) out_counts[p * nf + f] = tot;
    }
    if (t == 0) status[p] = 0;
}

}  // namespace

extern "C" int dodt_three_d_iou_matrix(dodt_ctx* ctx, const double* d_a, int na, const double* d_b, int nb,
                                       double* d_iou_out) {
    DODT_REQUIRE(ctx && na >= 0 && nb >= 0, "dodt_three_d_iou_matrix: bad arguments");
    const long long n = (long long)na * nb;
    if (n == 0) return DODT_OK;
    DODT_REQUIRE(d_a && d_b && d_iou_out, "dodt_three_d_iou_matrix: NULL argument");
    hipLaunchKernelGGL(iou_matrix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_a, na, d_b,
                       nb, d_iou_out);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

namespace {

template <typename T, typename CalibArg>
int launch_interpolate(dodt_ctx* ctx, const void* d_records, const int32_t* d_counts, int n_pairs, int max_det,
                       int n_frames, double threshold, int nb, const double* d_recover, CalibArg calib, int max_out,
                       size_t lds, const double* ws, double* d_out, int32_t* d_out_counts, int32_t* d_status) {
    static bool attr_set = false;       // (per instantiation)
    if (!attr_set) {
        DODT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&interpolate_kernel<T, CalibArg>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        attr_set = true;
    }
    hipLaunchKernelGGL((interpolate_kernel<T, CalibArg>), dim3(n_pairs), dim3(kThreads), lds, ctx->stream,
                       static_cast<const T*>(d_records), d_counts, max_det, n_frames, threshold, nb, d_recover, calib,
                       max_out, ws, d_out, d_out_counts, d_status);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

// Both entries: `calib` the 42 host doubles of dodt_interpolate_pairs (or NULL), or d_calibs the (n_pairs, 42) device
// rows of dodt_interpolate_pairs_calibs.
int interpolate_pairs(const char* who, dodt_ctx* ctx, const void* d_records, int records_f64, const int32_t* d_counts,
                      int n_pairs, int max_det, int n_frames, double threshold, int on_conflict,
                      const double* d_recover, const double* calib, const double* d_calibs, int max_out, double* d_out,
                      int32_t* d_out_counts, int32_t* d_status) {
    DODT_REQUIRE(ctx && n_pairs >= 0, "%s: bad arguments", who);
    if (n_pairs == 0) return DODT_OK;
    DODT_REQUIRE(d_records && d_counts && d_out && d_out_counts && d_status, "%s: NULL argument", who);
    DODT_REQUIRE(max_det >= 1 && max_det <= kMaxDet, "%s: max_det %d outside 1..%d", who, max_det, kMaxDet);
    DODT_REQUIRE(n_frames >= 1 && n_frames <= kMaxFrames, "%s: n_frames %d outside 1..%d", who, n_frames, kMaxFrames);
    DODT_REQUIRE(max_out >= 2 * max_det, "%s: max_out %d below 2 * max_det", who, max_out);
    DODT_REQUIRE(on_conflict == DODT_CONFLICT_RAISE || on_conflict == DODT_CONFLICT_NEXT_BEST,
                 "%s: on_conflict must be DODT_CONFLICT_RAISE or DODT_CONFLICT_NEXT_BEST", who);
    DODT_REQUIRE(!d_recover || calib || d_calibs, "%s: d_recover needs a calibration", who);
    Calib k;
    memset(&k, 0, sizeof(k));
    if (calib) memcpy(&k, calib, sizeof(k));
    const bool assoc = n_frames >= 3;
    const size_t lds = assoc ? (size_t)max_det * max_det * sizeof(double) : 0;
    double* ws = nullptr;
    if (assoc) {
        if (ctx->temporal_ws.reserve((size_t)n_pairs * max_det * max_det * sizeof(double)) != DODT_OK) return DODT_ERR_HIP;
        ws = static_cast<double*>(ctx->temporal_ws.ptr);
        const dim3 grid((unsigned)dodt::ceil_div(max_det * max_det, 256), (unsigned)n_pairs);
        if (records_f64)
            hipLaunchKernelGGL(pair_iou_kernel<double>, grid, dim3(256), 0, ctx->stream,
                               static_cast<const double*>(d_records), d_counts, max_det, threshold, ws);
        else
            hipLaunchKernelGGL(pair_iou_kernel<float>, grid, dim3(256), 0, ctx->stream,
                               static_cast<const float*>(d_records), d_counts, max_det, threshold, ws);
        DODT_LAUNCH_CHECK();
    }
    const int nb = on_conflict == DODT_CONFLICT_NEXT_BEST;
    if (d_calibs) {
        const Calib* rows = reinterpret_cast<const Calib*>(d_calibs);
        return records_f64
            ? launch_interpolate<double, const Calib*>(ctx, d_records, d_counts, n_pairs, max_det, n_frames, threshold,
                                                        nb, d_recover, rows, max_out, lds, ws, d_out, d_out_counts, d_status)
            : launch_interpolate<float, const Calib*>(ctx, d_records, d_counts, n_pairs, max_det, n_frames, threshold,
                                                       nb, d_recover, rows, max_out, lds, ws, d_out, d_out_counts, d_status);
    }
    return records_f64
        ? launch_interpolate<double, Calib>(ctx, d_records, d_counts, n_pairs, max_det, n_frames, threshold, nb,
                                            d_recover, k, max_out, lds, ws, d_out, d_out_counts, d_status)
        : launch_interpolate<float, Calib>(ctx, d_records, d_counts, n_pairs, max_det, n_frames, threshold, nb,
                                           d_recover, k, max_out, lds, ws, d_out, d_out_counts, d_status);
}

}  // namespace

extern "C" int dodt_interpolate_pairs(dodt_ctx* ctx, const void* d_records, int records_f64, const int32_t* d_counts,
                                      int n_pairs, int max_det, int n_frames, double threshold, int on_conflict,
                                      const double* d_recover, const double* calib, int max_out, double* d_out,
                                      int32_t* d_out_counts, int32_t* d_status) {
    DODT_REQUIRE(!d_recover || calib, "dodt_interpolate_pairs: d_recover needs calib");
    return interpolate_pairs("dodt_interpolate_pairs", ctx, d_records, records_f64, d_counts, n_pairs, max_det, n_frames,
                             threshold, on_conflict, d_recover, calib, nullptr, max_out, d_out, d_out_counts, d_status);
}

extern "C" int dodt_interpolate_pairs_calibs(dodt_ctx* ctx, const void* d_records, int records_f64,
                                             const int32_t* d_counts, int n_pairs, int max_det, int n_frames,
                                             double threshold, int on_conflict, const double* d_recover,
                                             const double* d_calibs, int max_out, double* d_out, int32_t* d_out_counts,
                                             int32_t* d_status) {
    DODT_REQUIRE(d_recover && d_calibs, "dodt_interpolate_pairs_calibs: needs d_recover and d_calibs");
    return interpolate_pairs("dodt_interpolate_pairs_calibs", ctx, d_records, records_f64, d_counts, n_pairs, max_det,
                             n_frames, threshold, on_conflict, d_recover, nullptr, d_calibs, max_out, d_out,
                             d_out_counts, d_status);
}
