// The velocity-extrapolating greedy IoU tracker of the video-level association on the device
// (dodt_amd/experiments/video_detection_iou.py interpolate_by_track, which mirrors the reference's
// avod/experiments/video_detection_iou.py:413-470): the keyframes of a sequence -> tracks, the tracker state on the device.
//
// Three launches per batch of keyframes (at most kChunk; a larger batch is walked chunk by chunk), as kalman.hip:
//   encode_kernel   (records only) the keyframe tables of tracking.hip, one body (track_encode.h).
//   vt_iou_kernel   over the whole chip, one lane per (live track, detection) of the batch's FIRST keyframe: the
//                   detection's box moved into the track's frame (ego_moved_box, ego_transform.h), iou_3d in float64
//                   under this tracker's permutation -- the TRACK's box enters with l and h swapped --, kept as float64.
//                   A later keyframe's matrix depends on the step before it, so the step kernel computes it itself with
//                   the same device function.
//   vt_step_kernel  one workgroup: per keyframe the score filter, the greedy walk over the tracks in list order (wave 0:
//                   a masked cross-lane argmax ordered by IoU descending, index ascending), then one lane per track --
//                   match: speed, extend_len = 0, max_score, entry count; coast: the stride-step prediction loop with
//                   the cut and the finish test --, the new tracks, and the compaction of live / finished / log by the
//                   workgroup prefix scan, in the host's list order.
// Arithmetic dtype: the host does its box arithmetic in the dtype of the detections' boxes3d arrays and compares a score
// in the score's.  The rows are stored as float32 or float64; the caller says which dtype the host holds boxes3d and
// scores in (box_f64, score_f64): speed and prediction are computed in the boxes' dtype, a float32 sum rounded to
// float32 before it goes into the state's double slots, and a score is compared with a threshold rounded to the scores'
// dtype (as NumPy compares a float32 with a Python float).  The header keeps the scores' dtype for the finish test of a
// flush.  The IoU is float64 either way.  Builds with -ffp-contract=off.
// Lanes (dodt_vt_track_lanes): pair i of a step belongs to lane i, each lane with a state, an ego row, a calibration
// and an image size of its own -- the same three launches over a chunk of kLaneChunk lanes: the shared lanes encode
// (track_encode.h), vt_iou_lanes_kernel (grid.y = lane, lane i's matrix in slice i of the workspace) and
// vt_step_lanes_kernel (one workgroup per lane: the step's one body with n_kf = 1 on the lane's own state).  An
// inactive lane's workgroups return before they read or write anything.
// Every loop is bounded by the list sizes, by `stride` or by `extend_len`; nothing waits on another workgroup.
#include "common.h"
#include "ego_transform.h"
#include "iou3d.h"
#include "track_encode.h"

#include <cmath>
#include <cstddef>

namespace {

constexpr int kMaxLive = 256;                 // live tracks at the start of a keyframe (rows of the IoU matrix)
constexpr int kLiveSlots = kMaxLive + kRows;  // ... plus the new tracks of one keyframe, before the clamp
constexpr int kChunk = 16;                    // keyframes per launch triple
constexpr int kLaneChunk = 8;                 // lanes per launch triple (their constants fill the kernel arguments)
static_assert(kLaneChunk <= kChunk, "a chunk of lanes encodes into the workspace sized for kChunk pairs");
constexpr int kDet = 13;                      // a detection as doubles: boxes3d [h,w,l,x,y,z,ry], boxes2d (4), score,
                                              // class (col 0 of the row)
constexpr int kMaxStep = 4096;                // stride and extend_len: the bound of the prediction loop
constexpr int kStatusLog = 1, kStatusLive = 2, kStatusIou = 4;
constexpr int kHasSpeed = 1, kCut = 2;        // VtTrack::flags
static_assert(kMaxLive == kThreads && kRows <= 128, "one lane per live track, two detections per lane of a wave");

struct VtHeader {
    int32_t n_live, next_id, n_log, n_fin;
    int32_t keyframe, status, log_cap, n_k1;   // n_k1: rows of the kept keyframe-1 list, -1: none kept
    int32_t score_f64;                         // the scores' dtype of the last batch tracked: the finish test of a flush
    int32_t pad[7];
};
struct VtTrack {
    int32_t id, n_dets, extend_len, flags;     // n_dets: len(track['dets']); flags: kHasSpeed (a gap > 1 was matched),
    double max_score;                          // kCut (finished records: the trailing predictions were cut)
    double speed[3];                           // of x, z, ry
    double det[kDet];                          // the last entry
};
struct VtLog {
    int32_t id, keyframe, kind, row;    // kind 0: real (row = its index in the keyframe's list), 1: predicted (row -1)
    double det[kDet];
};
constexpr size_t kLiveOff = sizeof(VtHeader);
constexpr size_t kK1Off = kLiveOff + kLiveSlots * sizeof(VtTrack);
constexpr size_t kFinOff = kK1Off + kRows * kK1 * sizeof(float);
static_assert(sizeof(VtHeader) == 64 && sizeof(VtTrack) == 152 && sizeof(VtLog) == 120 && kFinOff % 8 == 0,
              "state layout (dodt_amd/tracking.py reads it)");

struct VtState {
    VtHeader* hdr;
    VtTrack* live;
    float* k1;
    VtTrack* fin;
    VtLog* log;
};
__device__ VtState vt_state_of(void* base, int cap) {
    char* b = static_cast<char*>(base);
    return {reinterpret_cast<VtHeader*>(b), reinterpret_cast<VtTrack*>(b + kLiveOff),
            reinterpret_cast<float*>(b + kK1Off), reinterpret_cast<VtTrack*>(b + kFinOff),
            reinterpret_cast<VtLog*>(b + kFinOff + (size_t)cap * sizeof(VtTrack))};
}

// The keyframe lists of a batch: 16-col KITTI rows (boxes2d 4:8, boxes3d 8:15, score 15), float32 or float64.
struct VtRows {
    const void* base;
    const int32_t* cnt;
    int f64, row_stride, cnt_stride, max_rows;
    size_t kf_stride;
};
__device__ int vt_count(const VtRows& r, int k) {
    return min(max(r.cnt[(size_t)k * r.cnt_stride], 0), min(r.max_rows, kRows));
}
__device__ double vt_col(const VtRows& r, int k, int i, int c) {
    const size_t at = (size_t)k * r.kf_stride + (size_t)i * r.row_stride + c;
    return r.f64 ? static_cast<const double*>(r.base)[at] : (double)static_cast<const float*>(r.base)[at];
}
__device__ void vt_load_det(const VtRows& r, int k, int i, double* det) {
    for (int c = 0; c < 7; ++c) det[c] = vt_col(r, k, i, 8 + c);
    for (int c = 0; c < 4; ++c) det[7 + c] = vt_col(r, k, i, 4 + c);
    det[11] = vt_col(r, k, i, 15);
    det[12] = vt_col(r, k, i, 0);
}

struct VtEgo {              // per keyframe of a chunk: trans (3), matrix (3x3, row major), delta -- the motion from the
    double e[kChunk][13];   // keyframe before it
};
struct VtParams {
    double sigma_l, sigma_h, sigma_iou;
    int t_min, extend_len, stride;
    int box_f64, score_f64;     // the dtype the host holds boxes3d / scores in: arithmetic and comparisons follow it
};
// The per-lane constants of a chunk of lanes, by value in the kernel arguments like VtEgo and KfCalib: read before the
// call returns, no upload, no lifetime.  440 bytes per lane; a launch's arguments are limited to 4 KB.
struct VtLane {
    double ego[13];         // the motion into the lane's current keyframe
    KfCalib cal;
};
struct VtLaneTable {
    VtLane a[kLaneChunk];
};
static_assert(sizeof(VtLane) == 440 && sizeof(VtLaneTable) + sizeof(VtRows) + sizeof(VtParams) + 64 <= 4096,
              "the step kernel's arguments: the lanes' table, the rows, the parameters and six words of pointers");
// lane i's keyframe as a batch of its own: the rows from list i on
__device__ VtRows vt_lane_rows(const VtRows& r, int i) {
    VtRows o = r;
    o.base = static_cast<const char*>(r.base) + (size_t)i * r.kf_stride * (r.f64 ? sizeof(double) : sizeof(float));
    o.cnt = r.cnt + (size_t)i * r.cnt_stride;
    return o;
}

// ---- arithmetic in the rows' dtype ---------------------------------------------------------------------------------
__device__ double vt_add(double a, double b, int f64) { return f64 ? a + b : (double)((float)a + (float)b); }
__device__ double vt_sub(double a, double b, int f64) { return f64 ? a - b : (double)((float)a - (float)b); }
__device__ bool vt_ge(double v, double thr, int f64) { return f64 ? v >= thr : (float)v >= (float)thr; }

// cal_transformed_ious: `det` [h,w,l,x,y,z,ry] moved into the frame of `last`, then this file's iou_3d: the reference
// hands the track's box over as [ry, h, l, w, ...] where [ry, l, h, w, ...] is read -- l and h swapped on that side
__device__ double vt_iou(const double* last, const double* det, const double* ego, const KfCalib& k) {
    const double a[7] = {last[3], last[4], last[5], last[0], last[1], last[2], last[6]};
    double b[7];
    ego_moved_box(det, ego, k, b);
    return iou_3d(a, b);
}

// the IoU matrix of keyframe k of `rows` against the live tracks: lane q of `n_lanes` strides over (track, row)
__device__ __forceinline__ void vt_matrix(const VtRows& rows, int k, const VtTrack* __restrict__ live, int nt,
                                          const double* ego, const KfCalib& cal, double* __restrict__ M, int q,
                                          int n_lanes) {
    const int nraw = vt_count(rows, k);
    for (; q < nt * nraw; q += n_lanes) {
        const int t = q / nraw, d = q % nraw;
        double det[kDet];
        vt_load_det(rows, k, d, det);
        M[(size_t)t * kRows + d] = vt_iou(live[t].det, det, ego, cal);
    }
}

// workgroup blockIdx.x's share of M (kMaxLive x kRows float64) of keyframe `k` of `rows` against the live tracks of `state`
__device__ __forceinline__ void vt_iou_state(const VtRows& rows, int k, const void* state, const double* ego,
                                             const KfCalib& cal, double* __restrict__ M) {
    const char* b = static_cast<const char*>(state);
    const VtHeader* h = reinterpret_cast<const VtHeader*>(b);
    const int nt = min(max(h->n_live, 0), kMaxLive);
    vt_matrix(rows, k, reinterpret_cast<const VtTrack*>(b + kLiveOff), nt, ego, cal, M,
              blockIdx.x * kThreads + threadIdx.x, gridDim.x * kThreads);
}

// M of keyframe `k` of the batch, over the whole chip
__global__ void __launch_bounds__(kThreads)
vt_iou_kernel(VtRows rows, int k, const void* state, VtEgo ego, KfCalib cal, double* __restrict__ M) {
    vt_iou_state(rows, k, state, ego.e[k], cal, M);
}

// Lanes: grid (kMaxLive * kRows / kThreads, lanes); lane blockIdx.y's keyframe against its OWN state under its own ego
// row and calibration, its matrix in slice blockIdx.y of M.
__global__ void __launch_bounds__(kThreads)
vt_iou_lanes_kernel(VtRows rows, unsigned mask, const char* __restrict__ states, size_t stride, VtLaneTable tab,
                    double* __restrict__ M) {
    const int i = blockIdx.y;
    if (!lane_on(mask, i)) return;
    vt_iou_state(vt_lane_rows(rows, i), 0, states + (size_t)i * stride, tab.a[i].ego, tab.a[i].cal,
                 M + (size_t)i * kMaxLive * kRows);
}

// (a, ja) comes before (b, jb): the larger IoU, on a tie the lower index (j < 0: no candidate)
__device__ bool vt_before(double a, int ja, double b, int jb) {
    if (ja < 0) return false;
    if (jb < 0) return true;
    if (a != b) return a > b;
    return ja < jb;
}

// The greedy association, run by ONE wave: the tracks 0..nt-1 in order, each takes the first maximum of its row of M
// over the detections still free (fdet[0:nd]: their columns; lane l owns detections l and l + 64) and matches it if
// that IoU is > thr.  trk2det[0:nt], det2trk[0:nd]: the partner or -1 (det2trk comes in as -1).  False if a candidate
// IoU was not finite.
__device__ bool vt_greedy_wave(const double* __restrict__ M, const int* fdet, int nt, int nd, double thr, int* trk2det,
                               int* det2trk) {
    const int lane = threadIdx.x & 63;
    bool free0 = lane < nd, free1 = lane + 64 < nd, finite = true;
    const int c0 = free0 ? fdet[lane] : 0, c1 = free1 ? fdet[lane + 64] : 0;
    for (int t = 0; t < nt; ++t) {
        const double* row = M + (size_t)t * kRows;
        double best = 0.0;
        int bj = -1;
        if (free0) {
            best = row[c0];
            bj = lane;
            if (!isfinite(best)) finite = false;
        }
        if (free1) {
            const double v = row[c1];
            if (!isfinite(v)) finite = false;
            if (vt_before(v, lane + 64, best, bj)) {
                best = v;
                bj = lane + 64;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off);
            const int oj = __shfl_xor(bj, off);
            if (vt_before(ov, oj, best, bj)) {
                best = ov;
                bj = oj;
            }
        }
        const int d = bj >= 0 && best > thr ? bj : -1;
        if (lane == 0) {
            trk2det[t] = d;
            if (d >= 0) det2trk[d] = t;
        }
        if (d == lane) free0 = false;
        if (d == lane + 64) free1 = false;
    }
    return !__any(!finite);
}

__device__ void vt_log_entry(VtLog* e, int id, int keyframe, int kind, int row, const double* det) {
    e->id = id;
    e->keyframe = keyframe;
    e->kind = kind;
    e->row = row;
    for (int c = 0; c < kDet; ++c) e->det[c] = det[c];
}

// One workgroup: keyframes 0..n_kf-1 of `rows` in order on `state`, keyframe k under the ego row ego + 13 k.  The one
// body of vt_step_kernel (a batch of one sequence) and vt_step_lanes_kernel (per workgroup a lane's view: one keyframe,
// its state).  M holds keyframe 0's matrix (vt_iou_kernel); the
// later ones are computed here.  k1 (or NULL): the keyframe-1 rows (kRows x 16 float32) and their count to keep in the
// state behind the batch.  kept: the batch is the state's own kept list (rows.base / rows.cnt point into it) -- skipped
// if none is kept, forgotten afterwards.  finish: then every live track with max_score >= sigma_h and >= t_min entries
// is finished, in order, its predictions not cut.
__device__ __forceinline__ void vt_step_keyframes(const VtRows& rows, int n_kf, void* state, double* __restrict__ M,
                                                  const double* ego, const KfCalib& cal, const VtParams& prm,
                                                  const float* __restrict__ k1, const int32_t* __restrict__ k1_cnt,
                                                  int kept, int finish) {
    __shared__ VtHeader h;
    __shared__ int fdet[kRows], det2trk[kRows], trk2det[kMaxLive], wave_tot[kThreads / 64], bad_iou;
    const int t = threadIdx.x, f64 = prm.box_f64, sf64 = prm.score_f64;
    VtState st = vt_state_of(state, 0);
    if (t == 0) {
        h = *st.hdr;
        bad_iou = 0;
    }
    __syncthreads();
    const int cap = h.log_cap;
    st = vt_state_of(state, cap);
    if (kept && h.n_k1 < 0) n_kf = 0;
    if (!kept && n_kf > 0 && t == 0) h.score_f64 = sf64;        // (a flush compares as the sequence's batches did)
    const int E = prm.extend_len, n_steps = min(prm.stride, E);

    for (int k = 0; k < n_kf; ++k) {
        const int nraw = vt_count(rows, k), nt = min(max(h.n_live, 0), kMaxLive), kf = h.keyframe, n_fin0 = h.n_fin;
        // ---- the detections with scores >= sigma_l, in order ---------------------------------------------------------
        const bool keep_d = t < nraw && vt_ge(vt_col(rows, k, t, 15), prm.sigma_l, sf64);
        int nd;
        const int dpos = block_scan(keep_d, wave_tot, &nd);
        if (keep_d) fdet[dpos] = t;
        if (t < kRows) det2trk[t] = -1;
        if (k > 0) vt_matrix(rows, k, st.live, nt, ego + 13 * k, cal, M, t, kThreads);
        __syncthreads();
        // ---- the greedy walk (wave 0) ---------------------------------------------------------------------------------
        if (t < 64) {
            const bool ok = vt_greedy_wave(M, fdet, nt, nd, prm.sigma_iou, trk2det, det2trk);
            if (!ok && t == 0) bad_iou = 1;
        }
        __syncthreads();
        // ---- one lane per live track: matched or coasting -------------------------------------------------------------
        VtTrack tr;
        bool matched = false, coasting = false;
        int row = -1, n_pred = 0;
        if (t < nt) {
            tr = st.live[t];
            const int d = trk2det[t];
            if (d >= 0) {
                matched = true;
                row = fdet[d];
                double nx[kDet];
                vt_load_det(rows, k, row, nx);
                if (prm.stride > 1) {       // (a frame gap of 1 leaves the speed alone)
                    tr.speed[0] = vt_sub(nx[3], tr.det[3], f64);
                    tr.speed[1] = vt_sub(nx[5], tr.det[5], f64);
                    tr.speed[2] = vt_sub(nx[6], tr.det[6], f64);
                    tr.flags |= kHasSpeed;
                }
                tr.n_dets += prm.stride;    // the frames in between and the detection
                tr.extend_len = 0;
                if (nx[11] > tr.max_score) tr.max_score = nx[11];
                for (int c = 0; c < kDet; ++c) tr.det[c] = nx[c];
            } else {
                coasting = true;
                n_pred = min(prm.stride, max(E - tr.extend_len, 0));
            }
        }
        int n_real, n_logged = 0;
        const int rpos = block_scan(matched, wave_tot, &n_real);
        if (matched && h.n_log + rpos < cap) vt_log_entry(st.log + h.n_log + rpos, tr.id, kf, 0, row, tr.det);
        n_logged += n_real;
        for (int i = 0; i < n_steps; ++i) {                     // predict_det's loop, one step of every coasting track
            const bool p = coasting && i < n_pred;
            if (p) {
                tr.det[3] = vt_add(tr.det[3], tr.speed[0], f64);
                tr.det[5] = vt_add(tr.det[5], tr.speed[1], f64);
                tr.det[6] = vt_add(tr.det[6], tr.speed[2], f64);
                tr.extend_len += 1;
                tr.n_dets += 1;
            }
            int n_p;
            const int ppos = block_scan(p, wave_tot, &n_p);
            const int at = h.n_log + n_logged + ppos;
            if (p && at < cap) vt_log_entry(st.log + at, tr.id, kf, 1, -1, tr.det);
            n_logged += n_p;
        }
        bool alive = matched, fin = false;
        if (coasting) {
            if (n_pred < prm.stride) {      // extend_len was reached inside the stride: cut the predictions, leave
                tr.n_dets -= E;
                tr.flags |= kCut;
                fin = vt_ge(tr.max_score, prm.sigma_h, sf64) && tr.n_dets >= prm.t_min;
            } else {
                alive = true;
            }
        }
        // ---- the lists, in the host's order: updated tracks, then a new track per free detection ----------------------
        int n_keep, n_new, n_f;
        const int kp = block_scan(alive, wave_tot, &n_keep);
        const int fp = block_scan(fin, wave_tot, &n_f);
        const bool opens = t < nd && det2trk[t] < 0;
        const int np = block_scan(opens, wave_tot, &n_new);
        if (alive) st.live[kp] = tr;        // (every lane read its track before the scans' barriers)
        if (fin && n_fin0 + fp < cap) st.fin[n_fin0 + fp] = tr;
        if (opens) {
            VtTrack nw;
            const int r = fdet[t];
            vt_load_det(rows, k, r, nw.det);
            nw.id = h.next_id + np;
            nw.n_dets = 1;
            nw.extend_len = 0;
            nw.flags = 0;
            nw.max_score = nw.det[11];
            nw.speed[0] = nw.speed[1] = nw.speed[2] = 0.0;
            st.live[n_keep + np] = nw;
            const int at = h.n_log + n_logged + np;
            if (at < cap) vt_log_entry(st.log + at, nw.id, kf, 0, r, nw.det);
        }
        __syncthreads();
        if (t == 0) {
            h.n_log += n_logged + n_new;
            h.n_fin = n_fin0 + n_f;
            if (h.n_log > cap || h.n_fin > cap) h.status |= kStatusLog;
            if (n_keep + n_new > kMaxLive) h.status |= kStatusLive;
            if (bad_iou) h.status |= kStatusIou;
            h.n_live = min(n_keep + n_new, kMaxLive);
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
        const int n_live = min(max(h.n_live, 0), kMaxLive), n_fin = h.n_fin;
        VtTrack e;
        bool fin = false;
        if (t < n_live) {
            e = st.live[t];
            fin = vt_ge(e.max_score, prm.sigma_h, h.score_f64) && e.n_dets >= prm.t_min;
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
vt_step_kernel(VtRows rows, int n_kf, void* state, double* __restrict__ M, VtEgo ego, KfCalib cal, VtParams prm,
               const float* __restrict__ k1, const int32_t* __restrict__ k1_cnt, int kept, int finish) {
    vt_step_keyframes(rows, n_kf, state, M, ego.e[0], cal, prm, k1, k1_cnt, kept, finish);
}

// Lanes: grid = lanes, one workgroup per lane; an inactive lane's workgroup leaves at once (the mask is uniform).  Lane
// i keeps ITS keyframe-1 rows (list i of k1, count cnt[i * kCnt + 1]) in its state.
__global__ void __launch_bounds__(kThreads)
vt_step_lanes_kernel(VtRows rows, unsigned mask, char* states, size_t stride, double* __restrict__ M, VtLaneTable tab,
                     VtParams prm, const float* __restrict__ k1, const int32_t* __restrict__ cnt) {
    const int i = blockIdx.x;
    if (!lane_on(mask, i)) return;
    vt_step_keyframes(vt_lane_rows(rows, i), 1, states + (size_t)i * stride, M + (size_t)i * kMaxLive * kRows,
                      tab.a[i].ego, tab.a[i].cal, prm, k1 + (size_t)i * kRows * kK1, cnt + (size_t)i * kCnt + 1, 0, 0);
}

__global__ void vt_reset_kernel(void* state, int cap) {
    if (threadIdx.x == 0) {
        VtHeader z{};
        z.log_cap = cap;
        z.n_k1 = -1;
        *static_cast<VtHeader*>(state) = z;
    }
}

// out (nt, nd) float64 = vt_iou(last[t], det[d]): boxes [h,w,l,x,y,z,ry] float64
__global__ void __launch_bounds__(kThreads)
vt_iou_boxes_kernel(const double* __restrict__ last, int nt, const double* __restrict__ det, int nd, VtEgo ego,
                    KfCalib cal, double* __restrict__ out) {
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= nt * nd) return;
    out[q] = vt_iou(last + (size_t)(q / nd) * 7, det + (size_t)(q % nd) * 7, ego.e[0], cal);
}

size_t vt_state_bytes(int cap) { return kFinOff + (size_t)cap * (sizeof(VtTrack) + sizeof(VtLog)); }

void vt_parked(double* e) {
    memset(e, 0, 13 * sizeof(double));
    e[3] = e[7] = e[11] = 1.0;
}

bool vt_params_ok(const VtParams& p) {
    return p.extend_len >= 1 && p.extend_len <= kMaxStep && p.stride >= 1 && p.stride <= kMaxStep;
}

// the launch pair of one chunk: keyframe 0's matrix over the chip, then the step
int vt_walk(dodt_ctx* ctx, void* d_state, const VtRows& rows, int n, const double* ego, const double* calib,
            const VtParams& prm, const float* k1, const int32_t* k1_cnt, int kept, int finish) {
    if (ctx->tracking_ws.reserve((size_t)kMaxLive * kRows * sizeof(double)) != DODT_OK) return DODT_ERR_HIP;
    double* M = static_cast<double*>(ctx->tracking_ws.ptr);
    VtEgo E;
    for (int k = 0; k < kChunk; ++k) {
        if (k < n && ego) memcpy(E.e[k], ego + (size_t)k * 13, sizeof(E.e[k]));
        else vt_parked(E.e[k]);
    }
    KfCalib cal;
    memcpy(&cal, calib, sizeof(cal));
    if (n > 0) {
        hipLaunchKernelGGL(vt_iou_kernel, dim3(kMaxLive * kRows / kThreads), dim3(kThreads), 0, ctx->stream, rows, 0,
                           static_cast<const void*>(d_state), E, cal, M);
        DODT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(vt_step_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, rows, n, d_state, M, E, cal, prm, k1,
                       k1_cnt, kept, finish);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

}  // namespace

extern "C" int dodt_vt_state_bytes(int log_capacity, size_t* bytes) {
    DODT_REQUIRE(log_capacity >= 1 && bytes, "dodt_vt_state_bytes: bad arguments");
    *bytes = vt_state_bytes(log_capacity);
    return DODT_OK;
}

extern "C" int dodt_vt_reset(dodt_ctx* ctx, void* d_state, int log_capacity) {
    DODT_REQUIRE(ctx && d_state && log_capacity >= 1, "dodt_vt_reset: bad arguments");
    hipLaunchKernelGGL(vt_reset_kernel, dim3(1), dim3(64), 0, ctx->stream, d_state, log_capacity);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

extern "C" int dodt_vt_track_keyframes(dodt_ctx* ctx, void* d_state, const void* d_rows, int rows_f64,
                                       const int32_t* d_counts, int n_keyframes, int max_rows, const double* ego,
                                       const double* calib, double sigma_l, double sigma_h, double sigma_iou,
                                       int t_min, int extend_len, int stride, int box_f64, int score_f64) {
    DODT_REQUIRE(ctx && d_state && n_keyframes >= 0, "dodt_vt_track_keyframes: bad arguments");
    DODT_REQUIRE(rows_f64 || (!box_f64 && !score_f64), "dodt_vt_track_keyframes: float64 values in float32 rows");
    const VtParams prm{sigma_l, sigma_h, sigma_iou, t_min, extend_len, stride, box_f64 != 0, score_f64 != 0};
    DODT_REQUIRE(vt_params_ok(prm), "dodt_vt_track_keyframes: extend_len %d, stride %d outside 1..%d", extend_len,
                 stride, kMaxStep);
    if (n_keyframes == 0) return DODT_OK;
    DODT_REQUIRE(d_rows && d_counts && ego && calib, "dodt_vt_track_keyframes: NULL argument");
    DODT_REQUIRE(max_rows >= 1 && max_rows <= kRows, "dodt_vt_track_keyframes: max_rows %d outside 1..%d", max_rows,
                 kRows);
    const size_t el = rows_f64 ? sizeof(double) : sizeof(float);
    for (int k0 = 0; k0 < n_keyframes; k0 += kChunk) {
        const int n = n_keyframes - k0 < kChunk ? n_keyframes - k0 : kChunk;
        const VtRows rows{static_cast<const char*>(d_rows) + (size_t)k0 * max_rows * kK1 * el, d_counts + k0,
                          rows_f64 != 0, kK1, 1, max_rows, (size_t)max_rows * kK1};
        const int rc = vt_walk(ctx, d_state, rows, n, ego + (size_t)k0 * 13, calib, prm, nullptr, nullptr, 0, 0);
        if (rc != DODT_OK) return rc;
    }
    return DODT_OK;
}

extern "C" int dodt_vt_track_pairs(dodt_ctx* ctx, void* d_state, const void* d_records, int records_f64,
                                   const int32_t* d_counts, int n_pairs, int max_det, const double* p2,
                                   double image_w, double image_h, double score_threshold, const double* ego,
                                   const double* calib, double sigma_l, double sigma_h, double sigma_iou, int t_min,
                                   int extend_len, int stride) {
    DODT_REQUIRE(ctx && d_state && n_pairs >= 0, "dodt_vt_track_pairs: bad arguments");
    const VtParams prm{sigma_l, sigma_h, sigma_iou, t_min, extend_len, stride, 0, 0};   // (encoded rows are float32)
    DODT_REQUIRE(vt_params_ok(prm), "dodt_vt_track_pairs: extend_len %d, stride %d outside 1..%d", extend_len, stride,
                 kMaxStep);
    if (n_pairs == 0) return DODT_OK;
    DODT_REQUIRE(d_records && d_counts && p2 && ego && calib, "dodt_vt_track_pairs: NULL argument");
    DODT_REQUIRE(max_det >= 1 && max_det <= kRows, "dodt_vt_track_pairs: max_det %d outside 1..%d", max_det, kRows);
    const size_t enc_bytes = (size_t)kChunk * kRows * (kTrk + kK1) * sizeof(float) + kChunk * kCnt * sizeof(int32_t);
    if (ctx->tracking_enc.reserve(enc_bytes) != DODT_OK) return DODT_ERR_HIP;
    float* trk = static_cast<float*>(ctx->tracking_enc.ptr);
    float* k1 = trk + (size_t)kChunk * kRows * kTrk;
    int32_t* cnt = reinterpret_cast<int32_t*>(k1 + (size_t)kChunk * kRows * kK1);
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
        const VtRows rows{trk, cnt + 3, 0, kTrk, kCnt, kRows, (size_t)kRows * kTrk};
        const int last = n - 1;
        const int rc = vt_walk(ctx, d_state, rows, n, ego + (size_t)p0 * 13, calib, prm,
                               k1 + (size_t)last * kRows * kK1, cnt + (size_t)last * kCnt + 1, 0, 0);
        if (rc != DODT_OK) return rc;
    }
    return DODT_OK;
}

extern "C" int dodt_vt_lanes_stride(int log_capacity, size_t* stride) {
    DODT_REQUIRE(log_capacity >= 1 && stride, "dodt_vt_lanes_stride: bad arguments");
    *stride = (vt_state_bytes(log_capacity) + 255) / 256 * 256;
    return DODT_OK;
}

extern "C" int dodt_vt_track_lanes(dodt_ctx* ctx, void* d_states, size_t stride, int n_lanes,
                                   const unsigned char* active, const void* d_records, int records_f64,
                                   const int32_t* d_counts, int max_det, const double* p2s, const double* image_whs,
                                   const double* egos, const double* calibs, double score_threshold, double sigma_l,
                                   double sigma_h, double sigma_iou, int t_min, int extend_len, int stride_frames) {
    DODT_REQUIRE(ctx && d_states && n_lanes >= 0, "dodt_vt_track_lanes: bad arguments");
    const VtParams prm{sigma_l, sigma_h, sigma_iou, t_min, extend_len, stride_frames, 0, 0};  // (encoded rows: float32)
    DODT_REQUIRE(vt_params_ok(prm), "dodt_vt_track_lanes: extend_len %d, stride %d outside 1..%d", extend_len,
                 stride_frames, kMaxStep);
    if (n_lanes == 0) return DODT_OK;
    DODT_REQUIRE(d_records && d_counts && p2s && image_whs && egos && calibs, "dodt_vt_track_lanes: NULL argument");
    DODT_REQUIRE(max_det >= 1 && max_det <= kRows, "dodt_vt_track_lanes: max_det %d outside 1..%d", max_det, kRows);
    DODT_REQUIRE(stride >= vt_state_bytes(1) && stride % alignof(VtTrack) == 0,
                 "dodt_vt_track_lanes: stride %zu is no distance between two states", stride);
    const size_t enc_bytes = (size_t)kChunk * kRows * (kTrk + kK1) * sizeof(float) + kChunk * kCnt * sizeof(int32_t);
    if (ctx->tracking_enc.reserve(enc_bytes) != DODT_OK) return DODT_ERR_HIP;
    if (ctx->tracking_ws.reserve((size_t)kLaneChunk * kMaxLive * kRows * sizeof(double)) != DODT_OK) return DODT_ERR_HIP;
    float* trk = static_cast<float*>(ctx->tracking_enc.ptr);
    float* k1 = trk + (size_t)kChunk * kRows * kTrk;
    int32_t* cnt = reinterpret_cast<int32_t*>(k1 + (size_t)kChunk * kRows * kK1);
    double* M = static_cast<double*>(ctx->tracking_ws.ptr);
    // lane i's keyframe: pair i's keyframe-0 rows (cols 0..15 of its track items, count in cnt[3])
    const VtRows rows{trk, cnt + 3, 0, kTrk, kCnt, kRows, (size_t)kRows * kTrk};
    const size_t rec_bytes = records_f64 ? sizeof(double) : sizeof(float);
    for (int l0 = 0; l0 < n_lanes; l0 += kLaneChunk) {
        const int n = n_lanes - l0 < kLaneChunk ? n_lanes - l0 : kLaneChunk;
        LaneCals<kLaneChunk> enc{};
        VtLaneTable tab{};
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
        hipLaunchKernelGGL(vt_iou_lanes_kernel, dim3(kMaxLive * kRows / kThreads, n), dim3(kThreads), 0, ctx->stream,
                           rows, mask, static_cast<const char*>(states), stride, tab, M);
        DODT_LAUNCH_CHECK();
        hipLaunchKernelGGL(vt_step_lanes_kernel, dim3(n), dim3(kThreads), 0, ctx->stream, rows, mask, states, stride, M,
                           tab, prm, static_cast<const float*>(k1), static_cast<const int32_t*>(cnt));
        DODT_LAUNCH_CHECK();
    }
    return DODT_OK;
}

extern "C" int dodt_vt_flush(dodt_ctx* ctx, void* d_state, const double* ego, const double* calib, double sigma_l,
                             double sigma_h, double sigma_iou, int t_min, int extend_len, int stride) {
    DODT_REQUIRE(ctx && d_state && calib, "dodt_vt_flush: bad arguments");
    const VtParams prm{sigma_l, sigma_h, sigma_iou, t_min, extend_len, stride, 0, 0};   // (the kept rows are float32)
    DODT_REQUIRE(vt_params_ok(prm), "dodt_vt_flush: extend_len %d, stride %d outside 1..%d", extend_len, stride,
                 kMaxStep);
    const char* b = static_cast<const char*>(d_state);
    const VtRows rows{b + kK1Off, reinterpret_cast<const int32_t*>(b + offsetof(VtHeader, n_k1)), 0, kK1, 0, kRows, 0};
    return vt_walk(ctx, d_state, rows, 1, ego, calib, prm, nullptr, nullptr, 1, 1);
}

extern "C" int dodt_vt_iou_matrix(dodt_ctx* ctx, const double* d_last, int n_tracks, const double* d_dets, int n_dets,
                                  const double* ego, const double* calib, double* d_iou_out) {
    DODT_REQUIRE(ctx && n_tracks >= 0 && n_dets >= 0 && calib, "dodt_vt_iou_matrix: bad arguments");
    if (n_tracks == 0 || n_dets == 0) return DODT_OK;
    DODT_REQUIRE(d_last && d_dets && d_iou_out, "dodt_vt_iou_matrix: NULL argument");
    VtEgo E;
    for (int k = 0; k < kChunk; ++k) vt_parked(E.e[k]);
    if (ego) memcpy(E.e[0], ego, sizeof(E.e[0]));
    KfCalib cal;
    memcpy(&cal, calib, sizeof(cal));
    const long long total = (long long)n_tracks * n_dets;
    DODT_REQUIRE(total <= (1ll << 30), "dodt_vt_iou_matrix: %d x %d too large", n_tracks, n_dets);
    hipLaunchKernelGGL(vt_iou_boxes_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       ctx->stream, d_last, n_tracks, d_dets, n_dets, E, cal, d_iou_out);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}
