// The Kalman-filter tracker of the video-level association on the device (dodt_amd/experiments/video_detection_kf.py
// kf_pipeline + dodt_amd/utils/kalman_tracker.py, which mirror the reference's avod/experiments/video_detection_kf.py
// and avod/utils/kalman_tracker.py): the keyframes of a sequence -> tracks of filtered positions, the tracker state on
// the device.
//
// Three launches per batch of keyframes (at most kChunk; a larger batch is walked chunk by chunk):
//   encode_kernel   (records only) the keyframe tables of tracking.hip, one body (track_encode.h).
//   kf_iou_kernel   over the whole chip, one lane per (live track, detection) of the batch's FIRST keyframe: the
//                   detection's box moved into the track's frame (label_transform_box), iou_3d in float64, stored as
//                   float32.  A later keyframe's matrix depends on the step before it (which tracks live, where the
//                   coasting ones were predicted to), so the step kernel computes it itself, with the same device
//                   function -- a pipeline step of one pair is the chip-wide case.
//   kf_step_kernel  one workgroup: per keyframe the score filter, the optimal assignment (wave 0, shortest augmenting
//                   paths), the gate, the filter one lane per track, `inside`, and the compaction of live / finished /
//                   log by the workgroup prefix scan.
// Lanes (dodt_kf_track_lanes): pair i of a step belongs to lane i, each lane with a state, an ego row, a calibration
// and an image size of its own -- the same three launches over a chunk of kLaneChunk lanes: the shared lanes encode
// (track_encode.h), kf_iou_lanes_kernel (grid.y = lane, lane i's matrix in slice i of the workspace) and
// kf_step_lanes_kernel (one workgroup per lane: the step's one body with n_kf = 1 on the lane's own state).  No
// workgroup waits for another; an inactive lane's workgroups return before they read or write anything.
// The ego rows and the calibration travel by value in the kernel arguments.  The filter and the IoU are float64;
// P stays block diagonal (F, Q, H, R are, and P0 = L I), so four 2x2 blocks and a diagonal S are the whole arithmetic.
// Builds with -ffp-contract=off.
#include "common.h"
#include "ego_transform.h"
#include "iou3d.h"
#include "track_encode.h"

#include <cmath>
#include <cstddef>

namespace {

constexpr int kMaxLive = 256;                 // live tracks at the start of a keyframe (rows of the IoU matrix)
constexpr int kLiveSlots = kMaxLive + kRows;  // ... plus the new tracks of one keyframe, before the drop
constexpr int kChunk = 16;                    // keyframes per launch triple
constexpr int kLaneChunk = 8;                 // lanes per launch triple (their constants fill the kernel arguments)
static_assert(kLaneChunk <= kChunk, "a chunk of lanes encodes into the workspace sized for kChunk pairs");
constexpr int kDet = 12;                      // a detection as doubles: boxes3d [h,w,l,x,y,z,ry], boxes2d (4), score
constexpr int kStatusLog = 1, kStatusLive = 2, kStatusSolver = 4;
static_assert(kMaxLive == kThreads, "one lane per live track");

struct KfHeader {
    int32_t n_live, next_id, n_log, n_fin;
    int32_t keyframe, status, log_cap, n_k1;   // n_k1: rows of the kept keyframe-1 list, -1: none kept
    int32_t pad[8];
};
struct KfTrack {
    int32_t id, hits, no_losses, last_kf;
    double x[8];            // [x, vx, y, vy, z, vz, ry, v_ry]
    double P[16];           // four 2x2 blocks [p00, p01, p10, p11]
    double det[kDet];       // the last detection (a coasting track's virtual one)
};
struct KfLog {
    int32_t id, keyframe, kind, row;    // kind 0: real (row = its index in the keyframe's list), 1: virtual (row -1)
    double det[kDet];
};
constexpr size_t kLiveOff = sizeof(KfHeader);
constexpr size_t kK1Off = kLiveOff + kLiveSlots * sizeof(KfTrack);
constexpr size_t kFinOff = kK1Off + kRows * kK1 * sizeof(float);
static_assert(sizeof(KfHeader) == 64 && sizeof(KfTrack) == 304 && sizeof(KfLog) == 112 && kFinOff % 8 == 0,
              "state layout (dodt_amd/tracking.py reads it)");

struct KfState {
    KfHeader* hdr;
    KfTrack* live;
    float* k1;
    KfTrack* fin;
    KfLog* log;
};
__device__ KfState kf_state_of(void* base, int cap) {
    char* b = static_cast<char*>(base);
    return {reinterpret_cast<KfHeader*>(b), reinterpret_cast<KfTrack*>(b + kLiveOff),
            reinterpret_cast<float*>(b + kK1Off), reinterpret_cast<KfTrack*>(b + kFinOff),
            reinterpret_cast<KfLog*>(b + kFinOff + (size_t)cap * sizeof(KfTrack))};
}

// The keyframe lists of a batch: 16-col KITTI rows (boxes2d 4:8, boxes3d 8:15, score 15), float32 or float64.
struct KfRows {
    const void* base;
    const int32_t* cnt;
    int f64, row_stride, cnt_stride, max_rows;
    size_t kf_stride;
};
__device__ int kf_count(const KfRows& r, int k) {
    return min(max(r.cnt[(size_t)k * r.cnt_stride], 0), min(r.max_rows, kRows));
}
__device__ double kf_col(const KfRows& r, int k, int i, int c) {
    const size_t at = (size_t)k * r.kf_stride + (size_t)i * r.row_stride + c;
    return r.f64 ? static_cast<const double*>(r.base)[at] : (double)static_cast<const float*>(r.base)[at];
}
__device__ void kf_load_det(const KfRows& r, int k, int i, double* det) {
    for (int c = 0; c < 7; ++c) det[c] = kf_col(r, k, i, 8 + c);
    for (int c = 0; c < 4; ++c) det[7 + c] = kf_col(r, k, i, 4 + c);
    det[11] = kf_col(r, k, i, 15);
}

struct KfEgo {              // per keyframe of a chunk: trans (3), matrix (3x3, row major), delta -- the motion from the
    double e[kChunk][13];   // keyframe before it
};
struct KfParams {
    double sigma_l, iou_thr, L, R;
    int max_age, min_hits;
};
// The per-lane constants of a chunk of lanes, by value in the kernel arguments like KfEgo and KfCalib: read before the
// call returns, no upload, no lifetime.  440 bytes per lane; a launch's arguments are limited to 4 KB.
struct KfLane {
    double ego[13];         // the motion into the lane's current keyframe
    KfCalib cal;
};
struct KfLaneTable {
    KfLane a[kLaneChunk];
};
static_assert(sizeof(KfLane) == 440 && sizeof(KfLaneTable) + sizeof(KfRows) + sizeof(KfParams) + 64 <= 4096,
              "the step kernel's arguments: the lanes' table, the rows, the parameters and six words of pointers");
// lane i's keyframe as a batch of its own: the rows from list i on
__device__ KfRows kf_lane_rows(const KfRows& r, int i) {
    KfRows o = r;
    o.base = static_cast<const char*>(r.base) + (size_t)i * r.kf_stride * (r.f64 ? sizeof(double) : sizeof(float));
    o.cnt = r.cnt + (size_t)i * r.cnt_stride;
    return o;
}

// cal_transformed_ious: `det` [h,w,l,x,y,z,ry] moved into the frame of `last` (ego_moved_box, ego_transform.h), then
// iou_3d under the host's permutation to [x,y,z,l,w,h,ry]
__device__ double kf_iou(const double* last, const double* det, const double* ego, const KfCalib& k) {
    const double a[7] = {last[3], last[4], last[5], last[2], last[1], last[0], last[6]};
    double b[7];
    ego_moved_box(det, ego, k, b);
    return iou_3d(a, b);
}

// ---- the filter (kalman_tracker.Tracker) ---------------------------------------------------------------------------
// x = F x, P = F P F' + Q per (position, rate) pair, dt = 1: F = [[1, 1], [0, 1]], Q = [[1/4, 1/2], [1/2, 1]]
__device__ void kf_predict(double* x, double* P) {
    for (int b = 0; b < 4; ++b) {
        x[2 * b] = x[2 * b] + x[2 * b + 1];
        double* p = P + 4 * b;
        const double a = p[0], bb = p[1], c = p[2], d = p[3];
        p[0] = ((a + c) + (bb + d)) + 0.25;
        p[1] = (bb + d) + 0.5;
        p[2] = (c + d) + 0.5;
        p[3] = d + 1.0;
    }
}
// S = H P H' + R (diagonal), K = P H' S^-1, x += K (z - H x), P -= K H P; after kf_predict
__device__ void kf_update(double* x, double* P, const double* z, double R) {
    for (int b = 0; b < 4; ++b) {
        double* p = P + 4 * b;
        const double inv = 1.0 / (p[0] + R);
        const double k0 = p[0] * inv, k1 = p[2] * inv;
        const double y = z[b] - x[2 * b];
        x[2 * b] = x[2 * b] + k0 * y;
        x[2 * b + 1] = x[2 * b + 1] + k1 * y;
        const double p00 = p[0], p01 = p[1];
        p[0] = p[0] - k0 * p00;
        p[1] = p[1] - k0 * p01;
        p[2] = p[2] - k1 * p00;
        p[3] = p[3] - k1 * p01;
    }
}
__device__ void kf_init(double* x, double* P, const double* z, double L) {
    for (int b = 0; b < 4; ++b) {
        x[2 * b] = z[b];
        x[2 * b + 1] = 0.0;
        P[4 * b] = L;
        P[4 * b + 1] = 0.0;
        P[4 * b + 2] = 0.0;
        P[4 * b + 3] = L;
    }
}
// what the reference feeds the filter: x, y, z and z again in the heading slot
__device__ void kf_meas(const double* det, double* z) {
    z[0] = det[3];
    z[1] = det[4];
    z[2] = det[5];
    z[3] = det[5];
}
// the box centre lies in 0 < z < 70, |x| < 40 and inside the wedge z > 1.3 |x|
__device__ bool kf_inside(const double* det) {
    const double x = det[3], z = det[5];
    return 0 < z && z < 70 && -40 < x && x < 40 && z + 1.3 * x > 0 && z - 1.3 * x > 0;
}

// ---- the assignment ------------------------------------------------------------------------------------------------
struct Solver {
    double u[kRows], v[kMaxLive], spc[kMaxLive];
    int path[kMaxLive], row4col[kMaxLive], col4row[kRows], sr[kRows];
    unsigned char sc[kMaxLive];
};
// one wave works on the solver's LDS arrays: a write of one lane is read by another behind this
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// the smaller cost; on a tie an unassigned column first, then the lower index (j < 0: no candidate)
__device__ bool sap_better(double a, int ja, bool fa, double b, int jb, bool fb) {
    if (ja < 0) return false;
    if (jb < 0) return true;
    if (a != b) return a < b;
    if (fa != fb) return fa;
    return ja < jb;
}

// The optimal assignment of the nt x nd matrix M (row stride ld; column d is M's column cols[d], or d): maximum total,
// costs the negated float32 entries widened to double.  Shortest augmenting paths over the smaller side (rectangular
// Jonker-Volgenant), run by ONE wave: the columns spread over its 64 lanes, the minimum by cross-lane shuffles, the
// duals and the path in LDS -- no __syncthreads().  trk2det[0:nt], det2trk[0:nd]: the partner or -1.  False if no
// finite path exists (a NaN matrix): nothing is assigned.
__device__ bool sap_assign_wave(const float* __restrict__ M, int ld, const int* cols, int nt, int nd, Solver& s,
                                int* trk2det, int* det2trk) {
    const int lane = threadIdx.x & 63;
    const bool tr = nt > nd;
    const int nr = tr ? nd : nt, nc = tr ? nt : nd;
    auto cost = [&](int i, int j) -> double {
        const int t = tr ? j : i, d = tr ? i : j;
        return -(double)M[(size_t)t * ld + (cols ? cols[d] : d)];
    };
    for (int j = lane; j < nc; j += 64) {
        s.v[j] = 0.0;
        s.row4col[j] = -1;
    }
    for (int i = lane; i < nr; i += 64) {
        s.u[i] = 0.0;
        s.col4row[i] = -1;
    }
    for (int t = lane; t < nt; t += 64) trk2det[t] = -1;
    for (int d = lane; d < nd; d += 64) det2trk[d] = -1;
    wave_sync();
    bool ok = true;
    for (int cur = 0; cur < nr && ok; ++cur) {
        for (int j = lane; j < nc; j += 64) {
            s.spc[j] = INFINITY;
            s.sc[j] = 0;
        }
        wave_sync();
        double min_val = 0.0;
        int i = cur, sink = -1, n_sr = 0;
        for (int it = 0; it < nc && sink < 0; ++it) {       // every turn closes one column
            if (lane == 0 && n_sr < kRows) s.sr[n_sr] = i;
            ++n_sr;
            const double ui = s.u[i];
            double best = INFINITY;
            int bj = -1;
            bool bfree = false;
            for (int j = lane; j < nc; j += 64) {
                if (s.sc[j]) continue;
                const double r = min_val + cost(i, j) - ui - s.v[j];
                if (r < s.spc[j]) {
                    s.path[j] = i;
                    s.spc[j] = r;
                }
                const double sp = s.spc[j];
                const bool fr = s.row4col[j] < 0;
                if (sap_better(sp, j, fr, best, bj, bfree)) {
                    best = sp;
                    bj = j;
                    bfree = fr;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const double ov = __shfl_xor(best, off);
                const int oj = __shfl_xor(bj, off);
                const bool of = __shfl_xor((int)bfree, off) != 0;
                if (sap_better(ov, oj, of, best, bj, bfree)) {
                    best = ov;
                    bj = oj;
                    bfree = of;
                }
            }
            if (bj < 0 || !(best < INFINITY)) {
                ok = false;
                break;
            }
            min_val = best;
            if (bfree) sink = bj;
            else i = s.row4col[bj];
            if (lane == 0) s.sc[bj] = 1;
            wave_sync();
        }
        if (!ok || sink < 0) {
            ok = false;
            break;
        }
        n_sr = min(n_sr, kRows);
        for (int k = lane; k < n_sr; k += 64) {             // the duals of the rows and columns the search reached
            const int r = s.sr[k], c = s.col4row[r];
            s.u[r] += r == cur || c < 0 ? min_val : min_val - s.spc[c];
        }
        for (int j = lane; j < nc; j += 64)
            if (s.sc[j]) s.v[j] -= min_val - s.spc[j];
        wave_sync();
        if (lane == 0) {                                    // augment along the path back to row `cur`
            int j = sink;
            for (int g = 0; g <= nr; ++g) {
                const int r = s.path[j];
                s.row4col[j] = r;
                const int pj = s.col4row[r];
                s.col4row[r] = j;
                j = pj;
                if (r == cur || j < 0) break;
            }
        }
        wave_sync();
    }
    if (ok)
        for (int i = lane; i < nr; i += 64) {
            const int j = s.col4row[i];
            const int t = tr ? j : i, d = tr ? i : j;
            trk2det[t] = d;
            det2trk[d] = t;
        }
    wave_sync();
    return ok;
}

// The gate over the workgroup: an assigned pair whose IoU is < thr is unmatched on both sides (trk2det[t] <- -1).
// newdet[0:n]: the detections that start a track, in the host's order -- those no row was assigned to, ascending,
// then the gate-failed ones in ascending track order.  Returns n.  Every lane calls it.
__device__ int kf_gate(const float* __restrict__ M, int ld, const int* cols, int nt, int nd, double thr, int* trk2det,
                       const int* det2trk, int* newdet, int* wave_tot) {
    const int t = threadIdx.x;
    const bool un = t < nd && det2trk[t] < 0;
    int u1, u2;
    int pos = block_scan(un, wave_tot, &u1);
    if (un) newdet[pos] = t;
    bool fail = false;
    int d = -1;
    if (t < nt) {
        d = trk2det[t];
        if (d >= 0) fail = (double)M[(size_t)t * ld + (cols ? cols[d] : d)] < thr;
    }
    pos = block_scan(fail, wave_tot, &u2);
    if (fail) {
        newdet[u1 + pos] = d;
        trk2det[t] = -1;
    }
    __syncthreads();
    return u1 + u2;
}

// the IoU matrix of keyframe k of `rows` against the live tracks: lane q of `n_lanes` strides over (track, row)
__device__ __forceinline__ void kf_matrix(const KfRows& rows, int k, const KfTrack* __restrict__ live, int nt,
                                          const double* ego, const KfCalib& cal, float* __restrict__ M, int q,
                                          int n_lanes) {
    const int nraw = kf_count(rows, k);
    for (; q < nt * nraw; q += n_lanes) {
        const int t = q / nraw, d = q % nraw;
        double det[kDet];
        kf_load_det(rows, k, d, det);
        M[(size_t)t * kRows + d] = (float)kf_iou(live[t].det, det, ego, cal);
    }
}

// workgroup blockIdx.x's share of M (kMaxLive x kRows float32) of keyframe `k` of `rows` against the live tracks of `state`
__device__ __forceinline__ void kf_iou_state(const KfRows& rows, int k, const void* state, const double* ego,
                                             const KfCalib& cal, float* __restrict__ M) {
    const char* b = static_cast<const char*>(state);
    const KfHeader* h = reinterpret_cast<const KfHeader*>(b);
    const int nt = min(max(h->n_live, 0), kMaxLive);
    kf_matrix(rows, k, reinterpret_cast<const KfTrack*>(b + kLiveOff), nt, ego, cal, M,
              blockIdx.x * kThreads + threadIdx.x, gridDim.x * kThreads);
}

// M of keyframe `k` of the batch, over the whole chip
__global__ void __launch_bounds__(kThreads)
kf_iou_kernel(KfRows rows, int k, const void* state, KfEgo ego, KfCalib cal, float* __restrict__ M) {
    kf_iou_state(rows, k, state, ego.e[k], cal, M);
}

// Lanes: grid (kMaxLive * kRows / kThreads, lanes); lane blockIdx.y's keyframe against its OWN state under its own ego
// row and calibration, its matrix in slice blockIdx.y of M.
__global__ void __launch_bounds__(kThreads)
kf_iou_lanes_kernel(KfRows rows, unsigned mask, const char* __restrict__ states, size_t stride, KfLaneTable tab,
                    float* __restrict__ M) {
    const int i = blockIdx.y;
    if (!lane_on(mask, i)) return;
    kf_iou_state(kf_lane_rows(rows, i), 0, states + (size_t)i * stride, tab.a[i].ego, tab.a[i].cal,
                 M + (size_t)i * kMaxLive * kRows);
}

// One workgroup: keyframes 0..n_kf-1 of `rows` in order on `state`, keyframe k under the ego row ego + 13 k.  The one
// body of kf_step_kernel (a batch of one sequence) and kf_step_lanes_kernel (per workgroup a lane's view: one keyframe,
// its state).  M holds keyframe 0's matrix (kf_iou_kernel); the
// later ones are computed here.  k1 (or NULL): the keyframe-1 rows (kRows x 16 float32) and their count to keep in the
// state behind the batch.  kept: the batch is the state's own kept list (rows.base / rows.cnt point into it) -- skipped
// if none is kept, forgotten afterwards.  finish: then every live track with hits >= min_hits is finished, in order.
__device__ __forceinline__ void kf_step_keyframes(const KfRows& rows, int n_kf, void* state, float* __restrict__ M,
                                                  const double* ego, const KfCalib& cal, const KfParams& prm,
                                                  const float* __restrict__ k1, const int32_t* __restrict__ k1_cnt,
                                                  int kept, int finish) {
    __shared__ Solver sol;
    __shared__ KfHeader h;
    __shared__ int fdet[kRows], det2trk[kRows], newdet[kRows], trk2det[kMaxLive], wave_tot[kThreads / 64];
    const int t = threadIdx.x;
    KfState st = kf_state_of(state, 0);
    if (t == 0) h = *st.hdr;
    __syncthreads();
    const int cap = h.log_cap;
    st = kf_state_of(state, cap);
    if (kept && h.n_k1 < 0) n_kf = 0;

    for (int k = 0; k < n_kf; ++k) {
        const int nraw = kf_count(rows, k), nt = h.n_live, kf = h.keyframe;
        // ---- the detections with scores >= sigma_l, in order ---------------------------------------------------------
        const bool keep_d = t < nraw && kf_col(rows, k, t, 15) >= prm.sigma_l;
        int nd;
        const int dpos = block_scan(keep_d, wave_tot, &nd);
        if (keep_d) fdet[dpos] = t;
        if (k > 0) kf_matrix(rows, k, st.live, nt, ego + 13 * k, cal, M, t, kThreads);
        __syncthreads();
        // ---- assignment (wave 0) and gate -----------------------------------------------------------------------------
        if (nt > 0 && nd > 0) {
            if (t < 64) {
                const bool ok = sap_assign_wave(M, kRows, fdet, nt, nd, sol, trk2det, det2trk);
                if (!ok && t == 0) h.status |= kStatusSolver;
            }
        } else {
            if (t < nt) trk2det[t] = -1;
            if (t < nd) det2trk[t] = -1;
        }
        __syncthreads();
        const int n_new = kf_gate(M, kRows, fdet, nt, nd, prm.iou_thr, trk2det, det2trk, newdet, wave_tot);
        // ---- the filter, one lane per live track: matched or coasting ------------------------------------------------
        KfTrack tr;
        bool logs = false;
        int kind = 0, row = -1;
        if (t < nt) {
            tr = st.live[t];
            const int d = trk2det[t];
            if (d >= 0) {
                row = fdet[d];
                kf_load_det(rows, k, row, tr.det);
                double z[4];
                kf_meas(tr.det, z);
                kf_predict(tr.x, tr.P);
                kf_update(tr.x, tr.P, z, prm.R);
                tr.hits += 1;
                tr.no_losses = 0;
                tr.last_kf = kf;
                logs = true;
            } else {
                tr.no_losses += 1;
                kf_predict(tr.x, tr.P);
                if (!kf_inside(tr.det)) {
                    tr.no_losses = prm.max_age + 1;
                } else {                    // boxes3d[[3, 4, 5, 5]] = box: slot 5 takes the fourth filtered value
                    tr.det[3] = tr.x[0];
                    tr.det[4] = tr.x[2];
                    tr.det[5] = tr.x[6];
                    tr.last_kf = kf;
                    logs = true;
                    kind = 1;
                }
            }
        }
        int n_logged;
        const int lpos = block_scan(logs, wave_tot, &n_logged);
        if (t < nt) st.live[t] = tr;
        if (logs && h.n_log + lpos < cap) {
            KfLog* e = st.log + h.n_log + lpos;
            e->id = tr.id;
            e->keyframe = kf;
            e->kind = kind;
            e->row = row;
            for (int c = 0; c < kDet; ++c) e->det[c] = tr.det[c];
        }
        // ---- a new track per unmatched detection, ids in the list's order ----------------------------------------------
        if (t < n_new) {
            KfTrack nw;
            row = fdet[newdet[t]];
            kf_load_det(rows, k, row, nw.det);
            double z[4];
            kf_meas(nw.det, z);
            kf_init(nw.x, nw.P, z, prm.L);
            kf_predict(nw.x, nw.P);
            nw.id = h.next_id + t;
            nw.hits = 0;
            nw.no_losses = 0;
            nw.last_kf = kf;
            st.live[nt + t] = nw;
            const int at = h.n_log + n_logged + t;
            if (at < cap) {
                KfLog* e = st.log + at;
                e->id = nw.id;
                e->keyframe = kf;
                e->kind = 0;
                e->row = row;
                for (int c = 0; c < kDet; ++c) e->det[c] = nw.det[c];
            }
        }
        __syncthreads();
        // ---- finish and drop: the list is compacted in place (a track moves down or stays) ----------------------------
        const int total = nt + n_new;
        int n_keep = 0, n_fin = h.n_fin;
        for (int base = 0; base < kLiveSlots; base += kThreads) {
            const int idx = base + t;
            const bool valid = idx < total;
            KfTrack e;
            if (valid) e = st.live[idx];
            const bool keep = valid && e.no_losses <= prm.max_age;
            const bool fin = valid && !keep && e.hits >= prm.min_hits;
            int kt, ft;
            const int kp = block_scan(keep, wave_tot, &kt);
            const int fp = block_scan(fin, wave_tot, &ft);
            if (keep) st.live[n_keep + kp] = e;
            if (fin && n_fin + fp < cap) st.fin[n_fin + fp] = e;
            n_keep += kt;
            n_fin += ft;
            __syncthreads();
        }
        if (t == 0) {
            h.n_log += n_logged + n_new;
            if (h.n_log > cap || n_fin > cap) h.status |= kStatusLog;
            if (n_keep > kMaxLive) h.status |= kStatusLive;
            h.n_live = min(n_keep, kMaxLive);
            h.n_fin = n_fin;
            h.next_id += n_new;
            h.keyframe = kf + 1;
        }
        __syncthreads();
    }

    if (k1) {
        const int n1 = min(max(*k1_cnt, 0), kRows);
        for (int q = t; q < n1 * kK1; q += kThreads) st.k1[q] = k1[q];
        if (t == 0) h.n_k1 = n1;
    }
    if (kept && t == 0) h.n_k1 = -1;
    if (finish) {
        __syncthreads();
        const int n_live = h.n_live, n_fin = h.n_fin;
        KfTrack e;
        bool fin = false;
        if (t < n_live) {
            e = st.live[t];
            fin = e.hits >= prm.min_hits;
        }
        int ft;
        const int fp = block_scan(fin, wave_tot, &ft);
        if (fin && n_fin + fp < cap) st.fin[n_fin + fp] = e;
        if (t == 0) {
            if (n_fin + ft > cap) h.status |= kStatusLog;
            h.n_fin = n_fin + ft;
            h.n_live = 0;
        }
    }
    __syncthreads();
    if (t == 0) *st.hdr = h;
}

__global__ void __launch_bounds__(kThreads)
kf_step_kernel(KfRows rows, int n_kf, void* state, float* __restrict__ M, KfEgo ego, KfCalib cal, KfParams prm,
               const float* __restrict__ k1, const int32_t* __restrict__ k1_cnt, int kept, int finish) {
    kf_step_keyframes(rows, n_kf, state, M, ego.e[0], cal, prm, k1, k1_cnt, kept, finish);
}

// Lanes: grid = lanes, one workgroup per lane; an inactive lane's workgroup leaves at once (the mask is uniform).  Lane
// i keeps ITS keyframe-1 rows (list i of k1, count cnt[i * kCnt + 1]) in its state.
__global__ void __launch_bounds__(kThreads)
kf_step_lanes_kernel(KfRows rows, unsigned mask, char* states, size_t stride, float* __restrict__ M, KfLaneTable tab,
                     KfParams prm, const float* __restrict__ k1, const int32_t* __restrict__ cnt) {
    const int i = blockIdx.x;
    if (!lane_on(mask, i)) return;
    kf_step_keyframes(kf_lane_rows(rows, i), 1, states + (size_t)i * stride, M + (size_t)i * kMaxLive * kRows,
                      tab.a[i].ego, tab.a[i].cal, prm, k1 + (size_t)i * kRows * kK1, cnt + (size_t)i * kCnt + 1, 0, 0);
}

__global__ void kf_reset_kernel(void* state, int cap) {
    if (threadIdx.x == 0) {
        KfHeader z{};
        z.log_cap = cap;
        z.n_k1 = -1;
        *static_cast<KfHeader*>(state) = z;
    }
}

// ---- the parts alone -----------------------------------------------------------------------------------------------
// one lane per track: x0 (4) -> [x0, 0, ...], P0 = L0 I, R = R_scaler L (LR: [L0, L, R_scaler] -- the host class keeps
// the P of its construction when L is set afterwards), then its operations (0: predict, else predict + update with z)
__global__ void __launch_bounds__(kThreads)
kf_filter_steps_kernel(const double* __restrict__ x0, const int32_t* __restrict__ ops, const double* __restrict__ zs,
                       const int32_t* __restrict__ n_ops, const double* __restrict__ LR, int n, int max_ops,
                       double* __restrict__ x_out, double* __restrict__ P_out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const double R = LR[3 * i + 2] * LR[3 * i + 1];
    double x[8], P[16];
    kf_init(x, P, x0 + 4 * i, LR[3 * i]);
    const int m = min(max(n_ops[i], 0), max_ops);
    for (int k = 0; k < m; ++k) {
        const size_t at = (size_t)i * max_ops + k;
        kf_predict(x, P);
        if (ops[at]) kf_update(x, P, zs + at * 4, R);
        for (int c = 0; c < 8; ++c) x_out[at * 8 + c] = x[c];
        double* o = P_out + at * 64;
        for (int c = 0; c < 64; ++c) o[c] = 0.0;
        for (int b = 0; b < 4; ++b)
            for (int r = 0; r < 2; ++r)
                for (int c = 0; c < 2; ++c) o[(2 * b + r) * 8 + 2 * b + c] = P[4 * b + 2 * r + c];
    }
}

// matrix (nt, nd) float32 -> matches (k, 2) in ascending track order, the unmatched detections and the unmatched
// tracks in the host's order; counts [k, n_unmatched_dets, n_unmatched_tracks, solver failed]
__global__ void __launch_bounds__(kThreads)
kf_assign_kernel(const float* __restrict__ M, int nt, int nd, double gate, int32_t* __restrict__ matches,
                 int32_t* __restrict__ un_dets, int32_t* __restrict__ un_trks, int32_t* __restrict__ counts) {
    __shared__ Solver sol;
    __shared__ int det2trk[kRows], newdet[kRows], trk2det[kMaxLive], wave_tot[kThreads / 64], failed;
    const int t = threadIdx.x;
    if (t == 0) failed = 0;
    if (t < nt) trk2det[t] = -1;
    if (t < nd) det2trk[t] = -1;
    __syncthreads();
    if (nt > 0 && nd > 0 && t < 64) {
        const bool ok = sap_assign_wave(M, nd, nullptr, nt, nd, sol, trk2det, det2trk);
        if (!ok && t == 0) failed = 1;
    }
    __syncthreads();
    const bool raw_un = t < nt && trk2det[t] < 0;           // no column was assigned to the track
    const int n_ud = kf_gate(M, nd, nullptr, nt, nd, gate, trk2det, det2trk, newdet, wave_tot);
    if (t < n_ud) un_dets[t] = newdet[t];
    const bool gate_un = t < nt && trk2det[t] < 0 && !raw_un;
    const bool hit = t < nt && trk2det[t] >= 0;
    int n1, n2, nm;
    const int p1 = block_scan(raw_un, wave_tot, &n1);
    const int p2 = block_scan(gate_un, wave_tot, &n2);
    const int pm = block_scan(hit, wave_tot, &nm);
    if (raw_un) un_trks[p1] = t;
    if (gate_un) un_trks[n1 + p2] = t;
    if (hit) {
        matches[2 * pm] = t;
        matches[2 * pm + 1] = trk2det[t];
    }
    if (t == 0) {
        counts[0] = nm;
        counts[1] = n_ud;
        counts[2] = n1 + n2;
        counts[3] = failed;
    }
}

// out (nt, nd) float32 = kf_iou(last[t], det[d]): boxes [h,w,l,x,y,z,ry] float64
__global__ void __launch_bounds__(kThreads)
kf_iou_boxes_kernel(const double* __restrict__ last, int nt, const double* __restrict__ det, int nd, KfEgo ego,
                    KfCalib cal, float* __restrict__ out) {
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= nt * nd) return;
    out[q] = (float)kf_iou(last + (size_t)(q / nd) * 7, det + (size_t)(q % nd) * 7, ego.e[0], cal);
}

size_t kf_state_bytes(int cap) { return kFinOff + (size_t)cap * (sizeof(KfTrack) + sizeof(KfLog)); }

KfParams kf_params(double sigma_l, double iou_thr, int max_age, int min_hits, double L, double R_scaler) {
    return {sigma_l, iou_thr, L, R_scaler * L, max_age, min_hits};
}

void kf_parked(double* e) {
    memset(e, 0, 13 * sizeof(double));
    e[3] = e[7] = e[11] = 1.0;
}

// the launch pair of one chunk: keyframe 0's matrix over the chip, then the step
int kf_walk(dodt_ctx* ctx, void* d_state, const KfRows& rows, int n, const double* ego, const double* calib,
            const KfParams& prm, const float* k1, const int32_t* k1_cnt, int kept, int finish) {
    if (ctx->tracking_ws.reserve((size_t)kMaxLive * kRows * sizeof(float)) != DODT_OK) return DODT_ERR_HIP;
    float* M = static_cast<float*>(ctx->tracking_ws.ptr);
    KfEgo E;
    for (int k = 0; k < kChunk; ++k) {
        if (k < n && ego) memcpy(E.e[k], ego + (size_t)k * 13, sizeof(E.e[k]));
        else kf_parked(E.e[k]);
    }
    KfCalib cal;
    memcpy(&cal, calib, sizeof(cal));
    if (n > 0) {
        hipLaunchKernelGGL(kf_iou_kernel, dim3(kMaxLive * kRows / kThreads), dim3(kThreads), 0, ctx->stream, rows, 0,
                           static_cast<const void*>(d_state), E, cal, M);
        DODT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(kf_step_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, rows, n, d_state, M, E, cal, prm, k1,
                       k1_cnt, kept, finish);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

}  // namespace

extern "C" int dodt_kf_state_bytes(int log_capacity, size_t* bytes) {
    DODT_REQUIRE(log_capacity >= 1 && bytes, "dodt_kf_state_bytes: bad arguments");
    *bytes = kf_state_bytes(log_capacity);
    return DODT_OK;
}

extern "C" int dodt_kf_reset(dodt_ctx* ctx, void* d_state, int log_capacity) {
    DODT_REQUIRE(ctx && d_state && log_capacity >= 1, "dodt_kf_reset: bad arguments");
    hipLaunchKernelGGL(kf_reset_kernel, dim3(1), dim3(64), 0, ctx->stream, d_state, log_capacity);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

extern "C" int dodt_kf_track_keyframes(dodt_ctx* ctx, void* d_state, const double* d_rows, const int32_t* d_counts,
                                       int n_keyframes, int max_rows, const double* ego, const double* calib,
                                       double sigma_l, double iou_threshold, int max_age, int min_hits, double L,
                                       double R_scaler) {
    DODT_REQUIRE(ctx && d_state && n_keyframes >= 0, "dodt_kf_track_keyframes: bad arguments");
    if (n_keyframes == 0) return DODT_OK;
    DODT_REQUIRE(d_rows && d_counts && ego && calib, "dodt_kf_track_keyframes: NULL argument");
    DODT_REQUIRE(max_rows >= 1 && max_rows <= kRows, "dodt_kf_track_keyframes: max_rows %d outside 1..%d", max_rows,
                 kRows);
    const KfParams prm = kf_params(sigma_l, iou_threshold, max_age, min_hits, L, R_scaler);
    for (int k0 = 0; k0 < n_keyframes; k0 += kChunk) {
        const int n = n_keyframes - k0 < kChunk ? n_keyframes - k0 : kChunk;
        const KfRows rows{d_rows + (size_t)k0 * max_rows * kK1, d_counts + k0, 1, kK1, 1, max_rows,
                          (size_t)max_rows * kK1};
        const int rc = kf_walk(ctx, d_state, rows, n, ego + (size_t)k0 * 13, calib, prm, nullptr, nullptr, 0, 0);
        if (rc != DODT_OK) return rc;
    }
    return DODT_OK;
}

extern "C" int dodt_kf_track_pairs(dodt_ctx* ctx, void* d_state, const void* d_records, int records_f64,
                                   const int32_t* d_counts, int n_pairs, int max_det, const double* p2,
                                   double image_w, double image_h, double score_threshold, const double* ego,
                                   const double* calib, double sigma_l, double iou_threshold, int max_age,
                                   int min_hits, double L, double R_scaler) {
    DODT_REQUIRE(ctx && d_state && n_pairs >= 0, "dodt_kf_track_pairs: bad arguments");
    if (n_pairs == 0) return DODT_OK;
    DODT_REQUIRE(d_records && d_counts && p2 && ego && calib, "dodt_kf_track_pairs: NULL argument");
    DODT_REQUIRE(max_det >= 1 && max_det <= kRows, "dodt_kf_track_pairs: max_det %d outside 1..%d", max_det, kRows);
    const size_t enc_bytes = (size_t)kChunk * kRows * (kTrk + kK1) * sizeof(float) + kChunk * kCnt * sizeof(int32_t);
    if (ctx->tracking_enc.reserve(enc_bytes) != DODT_OK) return DODT_ERR_HIP;
    float* trk = static_cast<float*>(ctx->tracking_enc.ptr);
    float* k1 = trk + (size_t)kChunk * kRows * kTrk;
    int32_t* cnt = reinterpret_cast<int32_t*>(k1 + (size_t)kChunk * kRows * kK1);
    const KfParams prm = kf_params(sigma_l, iou_threshold, max_age, min_hits, L, R_scaler);
    P2 P;
    memcpy(P.p, p2, sizeof(P.p));
    const size_t rec_bytes = records_f64 ? sizeof(double) : sizeof(float);
    for (int p0 = 0; p0 < n_pairs; p0 += kChunk) {
        const int n = n_pairs - p0 < kChunk ? n_pairs - p0 : kChunk;
        const char* rec = static_cast<const char*>(d_records) + (size_t)p0 * 2 * max_det * kRecCols * rec_bytes;
        if (records_f64)
            hipLaunchKernelGGL(encode_kernel<double>, dim3(n), dim3(kThreads), 0, ctx->stream,
                               reinterpret_cast<const double*>(rec), d_counts + 2 * p0, max_det, P, image_w, image_h,
                               score_threshold, trk, k1, cnt);
        else
            hipLaunchKernelGGL(encode_kernel<float>, dim3(n), dim3(kThreads), 0, ctx->stream,
                               reinterpret_cast<const float*>(rec), d_counts + 2 * p0, max_det, P, image_w, image_h,
                               score_threshold, trk, k1, cnt);
        DODT_LAUNCH_CHECK();
        // keyframe j of the chunk: pair j's keyframe-0 rows (cols 0..15 of its track items, count in cnt[3])
        const KfRows rows{trk, cnt + 3, 0, kTrk, kCnt, kRows, (size_t)kRows * kTrk};
        const int last = n - 1;
        const int rc = kf_walk(ctx, d_state, rows, n, ego + (size_t)p0 * 13, calib, prm,
                               k1 + (size_t)last * kRows * kK1, cnt + (size_t)last * kCnt + 1, 0, 0);
        if (rc != DODT_OK) return rc;
    }
    return DODT_OK;
}

extern "C" int dodt_kf_lanes_stride(int log_capacity, size_t* stride) {
    DODT_REQUIRE(log_capacity >= 1 && stride, "dodt_kf_lanes_stride: bad arguments");
    *stride = (kf_state_bytes(log_capacity) + 255) / 256 * 256;
    return DODT_OK;
}

extern "C" int dodt_kf_track_lanes(dodt_ctx* ctx, void* d_states, size_t stride, int n_lanes,
                                   const unsigned char* active, const void* d_records, int records_f64,
                                   const int32_t* d_counts, int max_det, const double* p2s, const double* image_whs,
                                   const double* egos, const double* calibs, double score_threshold, double sigma_l,
                                   double iou_threshold, int max_age, int min_hits, double L, double R_scaler) {
    DODT_REQUIRE(ctx && d_states && n_lanes >= 0, "dodt_kf_track_lanes: bad arguments");
    if (n_lanes == 0) return DODT_OK;
    DODT_REQUIRE(d_records && d_counts && p2s && image_whs && egos && calibs, "dodt_kf_track_lanes: NULL argument");
    DODT_REQUIRE(max_det >= 1 && max_det <= kRows, "dodt_kf_track_lanes: max_det %d outside 1..%d", max_det, kRows);
    DODT_REQUIRE(stride >= kf_state_bytes(1) && stride % alignof(KfTrack) == 0,
                 "dodt_kf_track_lanes: stride %zu is no distance between two states", stride);
    const size_t enc_bytes = (size_t)kChunk * kRows * (kTrk + kK1) * sizeof(float) + kChunk * kCnt * sizeof(int32_t);
    if (ctx->tracking_enc.reserve(enc_bytes) != DODT_OK) return DODT_ERR_HIP;
    if (ctx->tracking_ws.reserve((size_t)kLaneChunk * kMaxLive * kRows * sizeof(float)) != DODT_OK) return DODT_ERR_HIP;
    float* trk = static_cast<float*>(ctx->tracking_enc.ptr);
    float* k1 = trk + (size_t)kChunk * kRows * kTrk;
    int32_t* cnt = reinterpret_cast<int32_t*>(k1 + (size_t)kChunk * kRows * kK1);
    float* M = static_cast<float*>(ctx->tracking_ws.ptr);
    const KfParams prm = kf_params(sigma_l, iou_threshold, max_age, min_hits, L, R_scaler);
    // lane i's keyframe: pair i's keyframe-0 rows (cols 0..15 of its track items, count in cnt[3])
    const KfRows rows{trk, cnt + 3, 0, kTrk, kCnt, kRows, (size_t)kRows * kTrk};
    const size_t rec_bytes = records_f64 ? sizeof(double) : sizeof(float);
    for (int l0 = 0; l0 < n_lanes; l0 += kLaneChunk) {
        const int n = n_lanes - l0 < kLaneChunk ? n_lanes - l0 : kLaneChunk;
        LaneCals<kLaneChunk> enc{};
        KfLaneTable tab{};
        unsigned mask = 0;
        for (int i = 0; i < n; ++i) {
            memcpy(enc.c[i].P.p, p2s + (size_t)(l0 + i) * 12, sizeof(enc.c[i].P.p));
            enc.c[i].iw = image_whs[2 * (l0 + i)];
            enc.c[i].ih = image_whs[2 * (l0 + i) + 1];
            memcpy(tab.a[i].ego, egos + (size_t)(l0 + i) * 13, sizeof(tab.a[i].ego));
            memcpy(&tab.a[i].cal, calibs + (size_t)(l0 + i) * 42, sizeof(KfCalib));
            if (!active || active[l0 + i]) mask |= 1u << i;
        }
        if (!mask) continue;
        const char* rec = static_cast<const char*>(d_records) + (size_t)l0 * 2 * max_det * kRecCols * rec_bytes;
        char* states = static_cast<char*>(d_states) + (size_t)l0 * stride;
        if (records_f64)
            hipLaunchKernelGGL((encode_lanes_kernel<double, kLaneChunk>), dim3(n), dim3(kThreads), 0, ctx->stream,
                               reinterpret_cast<const double*>(rec), d_counts + 2 * l0, max_det, enc, mask,
                               score_threshold, trk, k1, cnt);
        else
            hipLaunchKernelGGL((encode_lanes_kernel<float, kLaneChunk>), dim3(n), dim3(kThreads), 0, ctx->stream,
                               reinterpret_cast<const float*>(rec), d_counts + 2 * l0, max_det, enc, mask,
                               score_threshold, trk, k1, cnt);
        DODT_LAUNCH_CHECK();
        hipLaunchKernelGGL(kf_iou_lanes_kernel, dim3(kMaxLive * kRows / kThreads, n), dim3(kThreads), 0, ctx->stream,
                           rows, mask, static_cast<const char*>(states), stride, tab, M);
        DODT_LAUNCH_CHECK();
        hipLaunchKernelGGL(kf_step_lanes_kernel, dim3(n), dim3(kThreads), 0, ctx->stream, rows, mask, states, stride, M,
                           tab, prm, static_cast<const float*>(k1), static_cast<const int32_t*>(cnt));
        DODT_LAUNCH_CHECK();
    }
    return DODT_OK;
}

extern "C" int dodt_kf_flush(dodt_ctx* ctx, void* d_state, const double* ego, const double* calib, double sigma_l,
                             double iou_threshold, int max_age, int min_hits, double L, double R_scaler) {
    DODT_REQUIRE(ctx && d_state && calib, "dodt_kf_flush: bad arguments");
    const char* b = static_cast<const char*>(d_state);
    const KfRows rows{b + kK1Off, reinterpret_cast<const int32_t*>(b + offsetof(KfHeader, n_k1)), 0, kK1, 0, kRows, 0};
    return kf_walk(ctx, d_state, rows, 1, ego, calib,
                   kf_params(sigma_l, iou_threshold, max_age, min_hits, L, R_scaler), nullptr, nullptr, 1, 1);
}

extern "C" int dodt_kf_filter_steps(dodt_ctx* ctx, const double* d_x0, const int32_t* d_ops, const double* d_z,
                                    const int32_t* d_n_ops, const double* d_LR, int n_tracks, int max_ops,
                                    double* d_x_out, double* d_P_out) {
    DODT_REQUIRE(ctx && n_tracks >= 0 && max_ops >= 0, "dodt_kf_filter_steps: bad arguments");
    if (n_tracks == 0 || max_ops == 0) return DODT_OK;
    DODT_REQUIRE(d_x0 && d_ops && d_z && d_n_ops && d_LR && d_x_out && d_P_out, "dodt_kf_filter_steps: NULL argument");
    hipLaunchKernelGGL(kf_filter_steps_kernel, dim3((n_tracks + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       ctx->stream, d_x0, d_ops, d_z, d_n_ops, d_LR, n_tracks, max_ops, d_x_out, d_P_out);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

extern "C" int dodt_kf_assign(dodt_ctx* ctx, const float* d_iou, int n_tracks, int n_dets, double iou_threshold,
                              int32_t* d_matches, int32_t* d_unmatched_dets, int32_t* d_unmatched_tracks,
                              int32_t* d_counts) {
    DODT_REQUIRE(ctx && d_counts, "dodt_kf_assign: bad arguments");
    DODT_REQUIRE(n_tracks >= 0 && n_tracks <= kMaxLive && n_dets >= 0 && n_dets <= kRows,
                 "dodt_kf_assign: %d x %d outside %d x %d", n_tracks, n_dets, kMaxLive, kRows);
    DODT_REQUIRE((n_tracks == 0 || n_dets == 0 || (d_iou && d_matches)) && (n_dets == 0 || d_unmatched_dets) &&
                     (n_tracks == 0 || d_unmatched_tracks),
                 "dodt_kf_assign: NULL argument");
    hipLaunchKernelGGL(kf_assign_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, d_iou, n_tracks, n_dets,
                       iou_threshold, d_matches, d_unmatched_dets, d_unmatched_tracks, d_counts);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

extern "C" int dodt_kf_iou_matrix(dodt_ctx* ctx, const double* d_last, int n_tracks, const double* d_dets, int n_dets,
                                  const double* ego, const double* calib, float* d_iou_out) {
    DODT_REQUIRE(ctx && n_tracks >= 0 && n_dets >= 0 && calib, "dodt_kf_iou_matrix: bad arguments");
    if (n_tracks == 0 || n_dets == 0) return DODT_OK;
    DODT_REQUIRE(d_last && d_dets && d_iou_out, "dodt_kf_iou_matrix: NULL argument");
    KfEgo E;
    for (int k = 0; k < kChunk; ++k) kf_parked(E.e[k]);
    if (ego) memcpy(E.e[0], ego, sizeof(E.e[0]));
    KfCalib cal;
    memcpy(&cal, calib, sizeof(cal));
    const long long total = (long long)n_tracks * n_dets;
    DODT_REQUIRE(total <= (1ll << 30), "dodt_kf_iou_matrix: %d x %d too large", n_tracks, n_dets);
    hipLaunchKernelGGL(kf_iou_boxes_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       ctx->stream, d_last, n_tracks, d_dets, n_dets, E, cal, d_iou_out);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}
