// The IoU tracker of the temporal module on the device (dodt_amd/core/dt_evaluator_utils.py encode_tracking_dets +
// track_through_ious, which mirror the reference's avod/core/dt_evaluator_utils.py:368-511): the detection records of
// a sequence of keyframe pairs -> KITTI label rows -> tracks linked by 3-D IoU, with the tracker state on the device.
//
// Three launches per batch of pairs (at most kChunk; a larger batch is walked chunk by chunk):
//   encode_kernel     one workgroup per pair: kitti_label_table of keyframe 0, of keyframe 0 shifted by the
//                     correlation head (record cols 9:16) and of keyframe 1, each compacted in row order; the pair is
//                     skipped when keyframes 0 and 1 both encode to nothing.
//   iou_tables_kernel over the whole chip: every IoU the walk of a pair can read.  An active track at pair j was
//                     updated or created at the previous non-skipped pair i, so its last box is one of L(i)'s, where
//                     L(j) = [track items of j (zip of k0 and koff)] + [k1 of i]; the walk's columns are always L(j)'s
//                     boxes.  T(j) = IoU(offsets of L(i), boxes of L(j)), S(j) = IoU(k1 of i, boxes of L(j)) (the
//                     merge's two tables) -- they depend on the encoded rows of two consecutive pairs only, not on the
//                     tracker state.
//   walk_kernel       one workgroup: the step's pairs in order -- merge, argmax over the free columns, finish or drop,
//                     new tracks -- on the precomputed tables; the active list lives in LDS during the launch.
// Lanes (dodt_track_lanes): pair i of a batch belongs to lane i, each lane with a state, a calibration and an image size
// of its own -- the same three launches, the encode indexed by a by-value table of the lanes' calibrations, the tables
// and the walk over per-lane views (a batch of ONE pair against the lane's own state), one walk workgroup per lane.
// Float64 IoUs with the host's kitti-row permutation (ry <- z, l <-> h) and iou_3d of iou3d.h; float32 rows rounded to
// 3 decimals exactly as numpy rounds (rint(x * 1000) / 1000 in float64).  Builds with -ffp-contract=off.
#include "common.h"
#include "iou3d.h"
#include "track_encode.h"         // kitti_row, encode_pair, encode_kernel, encode_lanes_kernel, block_scan (shared)

#include <cfloat>
#include <climits>

namespace {

constexpr int kCols = 2 * kRows;  // columns of a pair: track items + the previous pair's keyframe-1 rows
constexpr int kChunk = 16;        // pairs per launch triple

struct Header {
    int32_t n_active, n_slots, n_log, n_fin;
    int32_t frame_num, seq_pair, status, has_prev;
    int32_t prev_pair, prev_nL, prev_n1, log_cap;
    int32_t pad[4];
};
struct Active {
    int32_t slot, row, len, start;
    float max_score;
    int32_t pad[3];
};
struct Finished {
    int32_t slot, start, len;
    float max_score;
};
struct LogEntry {
    int32_t slot, pair, kf, row;
    float v[16];        // the 16-col KITTI row
    float off[7];       // its 'offsets': the shifted box of a track item, a merged keyframe-1 row's own box
    int32_t pad;
};
constexpr size_t kActiveOff = sizeof(Header);
constexpr size_t kPrevOffOff = kActiveOff + kCols * sizeof(Active);
constexpr size_t kPrevK1Off = kPrevOffOff + kCols * 7 * sizeof(float);
constexpr size_t kFinOff = kPrevK1Off + kRows * kK1 * sizeof(float);
static_assert(sizeof(Header) == 64 && sizeof(Active) == 32 && sizeof(Finished) == 16 && sizeof(LogEntry) == 112,
              "state layout (dodt_amd/tracking.py reads it)");

struct State {
    Header* hdr;
    Active* act;
    float* prev_off;   // (kCols, 7): offsets of L(previous non-skipped pair)
    float* prev_k1;    // (kRows, 16): keyframe-1 rows of the previous non-skipped pair
    Finished* fin;
    LogEntry* log;
};

__device__ State state_of(void* base, int cap) {
    char* b = static_cast<char*>(base);
    State s;
    s.hdr = reinterpret_cast<Header*>(b);
    s.act = reinterpret_cast<Active*>(b + kActiveOff);
    s.prev_off = reinterpret_cast<float*>(b + kPrevOffOff);
    s.prev_k1 = reinterpret_cast<float*>(b + kPrevK1Off);
    s.fin = reinterpret_cast<Finished*>(b + kFinOff);
    s.log = reinterpret_cast<LogEntry*>(b + kFinOff + (size_t)cap * sizeof(Finished));
    return s;
}

struct Lists {              // encoded pairs: trk (n, rows, 23), k1 (n, rows, 16), cnt (n, cnt_stride)
    const float* trk;
    const float* k1;
    const int32_t* cnt;
    int cnt_stride, rows;
};

// The calibrations of a chunk of lanes, by value in the kernel arguments (kChunk * 112 = 1792 bytes; LaneCals,
// encode_lanes_kernel and lane_on of track_encode.h, shared with the other two trackers' lanes).
using LaneTable = LaneCals<kChunk>;

__device__ bool skipped(const Lists& ls, int p) { return ls.cnt_stride > 2 && ls.cnt[(size_t)p * ls.cnt_stride + 2]; }
__device__ int n_trk(const Lists& ls, int p) { return min(max(ls.cnt[(size_t)p * ls.cnt_stride], 0), ls.rows); }
__device__ int n_k1(const Lists& ls, int p) { return min(max(ls.cnt[(size_t)p * ls.cnt_stride + 1], 0), ls.rows); }
__device__ int pred_of(const Lists& ls, int p) {      // the previous non-skipped pair of the batch, or -1 (the state)
    for (int q = p - 1; q >= 0; --q)
        if (!skipped(ls, q)) return q;
    return -1;
}

// Where the keyframe-1 rows that L(p) appends come from: the pair before it in the batch, or the state.
struct K1Src {
    const float* rows;
    int n, pair_off;        // pair_off: batch index of the source, -1 for the state
};
__device__ K1Src k1_source(const Lists& ls, const Header& h, const float* prev_k1, int p) {
    const int q = pred_of(ls, p);
    if (q >= 0) return {ls.k1 + (size_t)q * ls.rows * kK1, n_k1(ls, q), q};
    return {prev_k1, h.has_prev ? h.prev_n1 : 0, -1};
}

// box c of L(p) ([h,w,l,x,y,z,ry] float32) as the kitti row three_d_iou takes: [x,y,z,h,w,l,z]
__device__ void kitti_box(const float* b, double* out) {
    out[0] = b[3];
    out[1] = b[4];
    out[2] = b[5];
    out[3] = b[0];
    out[4] = b[1];
    out[5] = b[2];
    out[6] = b[5];
}
__device__ const float* col_box(const Lists& ls, int p, int nt, const K1Src& src, int c) {
    return c < nt ? ls.trk + ((size_t)p * ls.rows + c) * kTrk + 8 : src.rows + (size_t)(c - nt) * kK1 + 8;
}

// lane i's pair as a batch of its own: the lists from pair i on
__device__ Lists lane_lists(const Lists& ls, int i) {
    return {ls.trk + (size_t)i * ls.rows * kTrk, ls.k1 + (size_t)i * ls.rows * kK1, ls.cnt + (size_t)i * ls.cnt_stride,
            ls.cnt_stride, ls.rows};
}

// workgroup blockIdx.x's share of T(p) and S(p) of pair p of the batch `ls`
__device__ __forceinline__ void iou_tables_pair(const Lists& ls, int p, const Header* __restrict__ hdr_p,
                                                const float* __restrict__ prev_off,
                                                const float* __restrict__ prev_k1, double* __restrict__ T,
                                                double* __restrict__ S) {
    if (skipped(ls, p)) return;
    const Header h = *hdr_p;
    const int nt = n_trk(ls, p);
    const K1Src src = k1_source(ls, h, prev_k1, p);
    const int nL = nt + src.n;
    const int q = blockIdx.x * kThreads + threadIdx.x;
    double a[7], b[7];
    if (blockIdx.x < kCols) {               // T: rows = offsets of L(pred)
        const int r = q / kCols, c = q % kCols;
        if (c >= nL) return;
        const int pq = src.pair_off;
        if (pq >= 0) {
            const int ntq = n_trk(ls, pq);
            const K1Src sq = k1_source(ls, h, prev_k1, pq);
            if (r >= ntq + sq.n) return;
            kitti_box(r < ntq ? ls.trk + ((size_t)pq * ls.rows + r) * kTrk + 16 : sq.rows + (size_t)(r - ntq) * kK1 + 8,
                      a);
        } else {
            if (!h.has_prev || r >= h.prev_nL) return;
            kitti_box(prev_off + (size_t)r * 7, a);
        }
        kitti_box(col_box(ls, p, nt, src, c), b);
        T[((size_t)p * kCols + r) * kCols + c] = iou_3d(a, b);
    } else {                                // S: rows = the keyframe-1 rows L(p) appends
        const int qq = q - kCols * kThreads;
        const int i = qq / kCols, c = qq % kCols;
        if (i >= src.n || c >= nL) return;
        kitti_box(col_box(ls, p, nt, src, nt + i), a);
        kitti_box(col_box(ls, p, nt, src, c), b);
        S[((size_t)p * kRows + i) * kCols + c] = iou_3d(a, b);
    }
}

// T(p) (kCols x kCols) and S(p) (kRows x kCols) of every pair of the batch; grid (kCols + kRows, n_pairs).
__global__ void __launch_bounds__(kThreads)
iou_tables_kernel(Lists ls, const Header* __restrict__ hdr_p, const float* __restrict__ prev_off,
                  const float* __restrict__ prev_k1, double* __restrict__ T, double* __restrict__ S) {
    iou_tables_pair(ls, blockIdx.y, hdr_p, prev_off, prev_k1, T, S);
}

// Lanes: grid (kCols + kRows, lanes); lane blockIdx.y is a batch of one pair against its OWN state (no pair of the
// batch precedes it: k1_source / pred_of always end at the state), its tables in slice blockIdx.y of T and S.
__global__ void __launch_bounds__(kThreads)
iou_tables_lanes_kernel(Lists ls, unsigned mask, const char* __restrict__ states, size_t stride,
                        double* __restrict__ T, double* __restrict__ S) {
    const int i = blockIdx.y;
    if (!lane_on(mask, i)) return;
    const char* b = states + (size_t)i * stride;
    iou_tables_pair(lane_lists(ls, i), 0, reinterpret_cast<const Header*>(b),
                    reinterpret_cast<const float*>(b + kPrevOffOff), reinterpret_cast<const float*>(b + kPrevK1Off),
                    T + (size_t)i * kCols * kCols, S + (size_t)i * kRows * kCols);
}

// np.argmax order: a NaN beats everything (the first NaN wins), otherwise the larger value, the first index on ties
__device__ bool better(double a, int ia, double b, int ib) {
    if (ib < 0) return ia >= 0;
    if (ia < 0) return false;
    const bool na = isnan(a), nb = isnan(b);
    if (na != nb) return na;
    if (!na && a != b) return a > b;
    return ia < ib;
}
__device__ void wave_argmax(double& v, int& i) {
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (better(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
}

__device__ bool alive_bit(const unsigned long long* m, int c) { return (m[c >> 6] >> (c & 63)) & 1ull; }

struct Item {               // a detection of L(p): its row and where it came from
    const float* row;       // 16 floats (track items: the keyframe-0 row)
    const float* off;       // 7 floats
    int pair, kf, idx;
};
__device__ Item item_of(const Lists& ls, int p, int nt, const K1Src& src, int seq_p, int prev_seq, int seq_base,
                        int L) {
    if (L < nt) {
        const float* r = ls.trk + ((size_t)p * ls.rows + L) * kTrk;
        return {r, r + 16, seq_p, 0, L};
    }
    const float* r = src.rows + (size_t)(L - nt) * kK1;
    return {r, r + 8, src.pair_off >= 0 ? seq_base + src.pair_off : prev_seq, 1, L - nt};
}

// lanes 0..22 of the calling wave write one log entry
__device__ void write_log(LogEntry* log, int idx, int slot, const Item& it, int lane) {
    LogEntry* e = log + idx;
    if (lane < 16) e->v[lane] = it.row[lane];
    else if (lane < 23) e->off[lane - 16] = it.off[lane - 16];
    if (lane == 0) {
        e->slot = slot;
        e->pair = it.pair;
        e->kf = it.kf;
        e->row = it.idx;
        e->pad = 0;         // (as a new track's entry: the log's bytes depend on the pairs alone, not on the buffer's past)
    }
}

// The walk of one workgroup: the n_pairs pairs of `ls` in order on `state`, with their tables T and S.  The one body
// of walk_kernel (a batch of one sequence) and walk_lanes_kernel (per workgroup a lane's view: one pair, its state).
__device__ __forceinline__ void walk_pairs(const Lists& ls, int n_pairs, void* state, const double* __restrict__ T,
                                           const double* __restrict__ S, double iou_thr, float high, int t_min) {
    __shared__ Active act[2][kCols];
    __shared__ int detL[kCols], colL[kCols], best_c[kCols];
    __shared__ double best_v[kCols];
    __shared__ unsigned long long among[kRows][2], alive_s[4];
    __shared__ int hits[kRows], wave_tot[kThreads / 64];
    __shared__ Header h;
    __shared__ int s_ncol, s_nu, s_last;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    State st = state_of(state, 0);
    if (t == 0) h = *st.hdr;
    __syncthreads();
    st = state_of(state, h.log_cap);
    const int cap = h.log_cap;
    for (int n = t; n < h.n_active; n += kThreads) act[0][n] = st.act[n];
    if (t == 0) s_last = -2;            // batch index of the last non-skipped pair (-2: none)
    const int seq_base = h.seq_pair;
    int cur = 0;
    __syncthreads();

    for (int p = 0; p < n_pairs; ++p) {
        if (skipped(ls, p)) continue;
        const int nt = n_trk(ls, p);
        const K1Src src = k1_source(ls, h, st.prev_k1, p);
        const int m = src.n, na = h.n_active;
        const double* Tp = T + (size_t)p * kCols * kCols;
        const double* Sp = S + (size_t)p * kRows * kCols;
        const Active* A = act[cur];
        Active* B = act[cur ^ 1];
        const bool merge = na > 0 && nt > 0 && m != nt;
        // ---- the columns: dets (what a match appends) and dets_iou (whose boxes the IoUs are taken with) ----------
        if (merge) {
            for (int i = w; i < m; i += kThreads / 64) {
                bool hit = false;
                for (int c = lane; c < nt; c += 64) hit |= Sp[(size_t)i * kCols + c] > 0;
                const unsigned long long a0 = __ballot(lane < m && Sp[(size_t)i * kCols + nt + lane] > 0);
                const unsigned long long a1 = __ballot(lane + 64 < m && Sp[(size_t)i * kCols + nt + 64 + lane] > 0);
                const bool any = __ballot(hit) != 0ull;
                if (lane == 0) {
                    hits[i] = any;
                    among[i][0] = a0;
                    among[i][1] = a1;
                }
            }
            for (int c = t; c < nt; c += kThreads) detL[c] = colL[c] = c;
            __syncthreads();
            if (t == 0) {                   // merge_dets: appended in order, each tested against the ones before it
                unsigned long long app[2] = {0ull, 0ull};
                int nc = nt;
                for (int i = 0; i < m; ++i)
                    if (!hits[i] && !(among[i][0] & app[0]) && !(among[i][1] & app[1])) {
                        app[i >> 6] |= 1ull << (i & 63);
                        detL[nc] = colL[nc] = nt + i;
                        ++nc;
                    }
                s_ncol = nc;
            }
        } else {
            const bool walked = na > 0 && nt > 0;   // equal lengths: the IoUs read dets_iou = the keyframe-1 rows
            for (int c = t; c < nt; c += kThreads) {
                detL[c] = c;
                colL[c] = walked ? nt + c : c;
            }
            if (t == 0) s_ncol = nt;
        }
        __syncthreads();
        const int ncol = s_ncol;
        // ---- each active track's argmax over all columns (one wave per track) ----------------------------------
        for (int n = w; n < na; n += kThreads / 64) {
            const double* row = Tp + (size_t)A[n].row * kCols;
            double bv = 0;
            int bi = -1;
            for (int c = lane; c < ncol; c += 64) {
                const double v = row[colL[c]];
                if (better(v, c, bv, bi)) {
                    bv = v;
                    bi = c;
                }
            }
            wave_argmax(bv, bi);
            if (lane == 0) {
                best_c[n] = bi;
                best_v[n] = bv;
            }
        }
        __syncthreads();
        // ---- the greedy walk over the active tracks, in order (wave 0) -----------------------------------------
        const int seq_p = seq_base + p;
        if (w == 0) {
            unsigned long long alive[4] = {0ull, 0ull, 0ull, 0ull};
            for (int c = 0; c < ncol; ++c) alive[c >> 6] |= 1ull << (c & 63);
            int nalive = ncol, nu = 0, n_log = h.n_log, n_fin = h.n_fin, status = h.status;
            for (int n = 0; n < na; ++n) {
                const Active tr = A[n];
                bool matched = false;
                int b = -1;
                if (nalive > 0) {
                    b = best_c[n];
                    double v = best_v[n];
                    if (!alive_bit(alive, b)) {     // its best column is taken: argmax over the free ones
                        const double* row = Tp + (size_t)tr.row * kCols;
                        double bv = 0;
                        int bi = -1;
                        for (int c = lane; c < ncol; c += 64)
                            if (alive_bit(alive, c)) {
                                const double x = row[colL[c]];
                                if (better(x, c, bv, bi)) {
                                    bv = x;
                                    bi = c;
                                }
                            }
                        wave_argmax(bv, bi);
                        b = bi;
                        v = bv;
                    }
                    matched = v > iou_thr;
                }
                if (matched) {
                    alive[b >> 6] &= ~(1ull << (b & 63));
                    --nalive;
                    const Item it = item_of(ls, p, nt, src, seq_p, h.prev_pair, seq_base, detL[b]);
                    const float sc = it.row[15];
                    if (lane == 0) {
                        Active u = tr;
                        u.row = detL[b];
                        u.len = tr.len + 1;
                        u.max_score = sc > tr.max_score ? sc : tr.max_score;    // Python's max(a, b)
                        B[nu] = u;
                    }
                    if (n_log < cap) write_log(st.log, n_log, tr.slot, it, lane);
                    else status |= 1;
                    ++n_log;
                    ++nu;
                } else if (tr.max_score >= high && tr.len >= t_min) {
                    if (n_fin < cap) {
                        if (lane == 0) st.fin[n_fin] = {tr.slot, tr.start, tr.len, tr.max_score};
                    } else {
                        status |= 1;
                    }
                    ++n_fin;
                }
            }
            if (lane == 0) {
                s_nu = nu;
                for (int k = 0; k < 4; ++k) alive_s[k] = alive[k];
                h.n_log = n_log;
                h.n_fin = n_fin;
                h.status = status;
            }
        }
        __syncthreads();
        // ---- new tracks: the detections no track took, in order --------------------------------------------------
        const bool fresh = t < ncol && alive_bit(alive_s, t);
        int tot;
        const int pos = block_scan(fresh, wave_tot, &tot);
        const int nu = s_nu;
        if (fresh) {
            const Item it = item_of(ls, p, nt, src, seq_p, h.prev_pair, seq_base, detL[t]);
            Active a;
            a.slot = h.n_slots + pos;
            a.row = detL[t];
            a.len = 1;
            a.start = h.frame_num;
            a.max_score = it.row[15];
            a.pad[0] = a.pad[1] = a.pad[2] = 0;
            B[nu + pos] = a;
            const int idx = h.n_log + pos;
            if (idx < cap) {
                LogEntry* e = st.log + idx;
                for (int c = 0; c < 16; ++c) e->v[c] = it.row[c];
                for (int c = 0; c < 7; ++c) e->off[c] = it.off[c];
                e->pad = 0;
                e->slot = a.slot;
                e->pair = it.pair;
                e->kf = it.kf;
                e->row = it.idx;
            }
        }
        __syncthreads();
        if (t == 0) {
            if (h.n_log + tot > cap) h.status |= 1;
            h.n_slots += tot;
            h.n_log += tot;
            h.n_active = nu + tot;
            h.frame_num += 1;
            h.has_prev = 1;
            h.prev_n1 = n_k1(ls, p);
            h.prev_nL = nt + m;
            s_last = p;
        }
        cur ^= 1;
        __syncthreads();
    }

    // ---- the state the next batch starts from ------------------------------------------------------------------------
    const int last = s_last;
    for (int n = t; n < h.n_active; n += kThreads) st.act[n] = act[cur][n];
    if (last >= 0) {
        // offsets of L(last): its track items' shifted boxes, then the appended keyframe-1 rows' own boxes.  The
        // latter may be the state's prev_k1: read all of them before writing any.
        Header h0 = *st.hdr;
        const int nt = n_trk(ls, last);
        const K1Src src = k1_source(ls, h0, st.prev_k1, last);
        float off[2][7];
        int k = 0;
        for (int r = t; r < kCols; r += kThreads, ++k)
            if (r < nt + src.n)
                for (int c = 0; c < 7; ++c)
                    off[k][c] = r < nt ? ls.trk[((size_t)last * ls.rows + r) * kTrk + 16 + c]
                                       : src.rows[(size_t)(r - nt) * kK1 + 8 + c];
        __syncthreads();
        k = 0;
        for (int r = t; r < kCols; r += kThreads, ++k)
            if (r < nt + src.n)
                for (int c = 0; c < 7; ++c) st.prev_off[(size_t)r * 7 + c] = off[k][c];
        const int n1 = n_k1(ls, last);
        for (int q = t; q < n1 * kK1; q += kThreads)
            st.prev_k1[q] = ls.k1[((size_t)last * ls.rows + q / kK1) * kK1 + q % kK1];
    }
    __syncthreads();
    if (t == 0) {
        if (last >= 0) h.prev_pair = seq_base + last;
        h.seq_pair = seq_base + n_pairs;
        *st.hdr = h;
    }
}

__global__ void __launch_bounds__(kThreads)
walk_kernel(Lists ls, int n_pairs, void* state, const double* __restrict__ T, const double* __restrict__ S,
            double iou_thr, float high, int t_min) {
    walk_pairs(ls, n_pairs, state, T, S, iou_thr, high, t_min);
}

// Lanes: grid = lanes, one workgroup per lane; an inactive lane's workgroup leaves at once (the mask is uniform).
__global__ void __launch_bounds__(kThreads)
walk_lanes_kernel(Lists ls, unsigned mask, char* states, size_t stride, const double* __restrict__ T,
                  const double* __restrict__ S, double iou_thr, float high, int t_min) {
    const int i = blockIdx.x;
    if (!lane_on(mask, i)) return;
    walk_pairs(lane_lists(ls, i), 1, states + (size_t)i * stride, T + (size_t)i * kCols * kCols,
               S + (size_t)i * kRows * kCols, iou_thr, high, t_min);
}

// finish the remaining active tracks, in order; the active list is emptied
__global__ void __launch_bounds__(kThreads) flush_kernel(void* state, float high, int t_min) {
    __shared__ int wave_tot[kThreads / 64];
    const int t = threadIdx.x;
    State st = state_of(state, 0);
    const Header h = *st.hdr;
    st = state_of(state, h.log_cap);
    Active a{};
    if (t < h.n_active) a = st.act[t];
    const bool fin = t < h.n_active && a.max_score >= high && a.len >= t_min;
    int tot;
    const int pos = block_scan(fin, wave_tot, &tot);
    if (fin && h.n_fin + pos < h.log_cap) st.fin[h.n_fin + pos] = {a.slot, a.start, a.len, a.max_score};
    __syncthreads();
    if (t == 0) {
        if (h.n_fin + tot > h.log_cap) st.hdr->status |= 1;
        st.hdr->n_fin = h.n_fin + tot;
        st.hdr->n_active = 0;
    }
}

__global__ void reset_kernel(void* state, int cap) {
    Header* h = static_cast<Header*>(state);
    if (threadIdx.x == 0) {
        Header z{};
        z.log_cap = cap;
        *h = z;
    }
}

size_t state_bytes(int cap) { return kFinOff + (size_t)cap * (sizeof(Finished) + sizeof(LogEntry)); }

int walk(dodt_ctx* ctx, void* d_state, const Lists& ls, int n_pairs, double high, double iou, int t_min) {
    if (ctx->tracking_ws.reserve((size_t)kChunk * (kCols + kRows) * kCols * sizeof(double)) != DODT_OK)
        return DODT_ERR_HIP;
    double* T = static_cast<double*>(ctx->tracking_ws.ptr);
    double* S = T + (size_t)kChunk * kCols * kCols;
    const Header* hdr = static_cast<const Header*>(d_state);
    const char* b = static_cast<const char*>(d_state);
    hipLaunchKernelGGL(iou_tables_kernel, dim3(kCols + kRows, n_pairs), dim3(kThreads), 0, ctx->stream, ls, hdr,
                       reinterpret_cast<const float*>(b + kPrevOffOff), reinterpret_cast<const float*>(b + kPrevK1Off),
                       T, S);
    DODT_LAUNCH_CHECK();
    hipLaunchKernelGGL(walk_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, ls, n_pairs, d_state, T, S, iou,
                       (float)high, t_min);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

int encode(dodt_ctx* ctx, const void* d_records, int records_f64, const int32_t* d_counts, int n_pairs, int max_det,
           const double* p2, double image_w, double image_h, double threshold, float* trk, float* k1, int32_t* cnt) {
    P2 P;
    memcpy(P.p, p2, sizeof(P.p));
    if (records_f64)
        hipLaunchKernelGGL(encode_kernel<double>, dim3(n_pairs), dim3(kThreads), 0, ctx->stream,
                           static_cast<const double*>(d_records), d_counts, max_det, P, image_w, image_h, threshold,
                           trk, k1, cnt);
    else
        hipLaunchKernelGGL(encode_kernel<float>, dim3(n_pairs), dim3(kThreads), 0, ctx->stream,
                           static_cast<const float*>(d_records), d_counts, max_det, P, image_w, image_h, threshold,
                           trk, k1, cnt);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

}  // namespace

extern "C" int dodt_track_state_bytes(int log_capacity, size_t* bytes) {
    DODT_REQUIRE(log_capacity >= 1 && bytes, "dodt_track_state_bytes: bad arguments");
    *bytes = state_bytes(log_capacity);
    return DODT_OK;
}

extern "C" int dodt_track_reset(dodt_ctx* ctx, void* d_state, int log_capacity) {
    DODT_REQUIRE(ctx && d_state && log_capacity >= 1, "dodt_track_reset: bad arguments");
    hipLaunchKernelGGL(reset_kernel, dim3(1), dim3(64), 0, ctx->stream, d_state, log_capacity);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

extern "C" int dodt_track_flush(dodt_ctx* ctx, void* d_state, double high_threshold, int t_min) {
    DODT_REQUIRE(ctx && d_state, "dodt_track_flush: bad arguments");
    hipLaunchKernelGGL(flush_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, d_state, (float)high_threshold, t_min);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

extern "C" int dodt_track_encode(dodt_ctx* ctx, const void* d_records, int records_f64, const int32_t* d_counts,
                                 int n_pairs, int max_det, const double* p2, double image_w, double image_h,
                                 double score_threshold, float* d_track_out, float* d_ious_out,
                                 int32_t* d_counts_out) {
    DODT_REQUIRE(ctx && n_pairs >= 0, "dodt_track_encode: bad arguments");
    if (n_pairs == 0) return DODT_OK;
    DODT_REQUIRE(d_records && d_counts && p2 && d_track_out && d_ious_out && d_counts_out,
                 "dodt_track_encode: NULL argument");
    DODT_REQUIRE(max_det >= 1 && max_det <= kRows, "dodt_track_encode: max_det %d outside 1..%d", max_det, kRows);
    return encode(ctx, d_records, records_f64, d_counts, n_pairs, max_det, p2, image_w, image_h, score_threshold,
                  d_track_out, d_ious_out, d_counts_out);
}

extern "C" int dodt_track_pairs(dodt_ctx* ctx, void* d_state, const void* d_records, int records_f64,
                                const int32_t* d_counts, int n_pairs, int max_det, const double* p2, double image_w,
                                double image_h, double score_threshold, double high_threshold, double iou_threshold,
                                int t_min) {
    DODT_REQUIRE(ctx && d_state && n_pairs >= 0, "dodt_track_pairs: bad arguments");
    if (n_pairs == 0) return DODT_OK;
    DODT_REQUIRE(d_records && d_counts && p2, "dodt_track_pairs: NULL argument");
    DODT_REQUIRE(max_det >= 1 && max_det <= kRows, "dodt_track_pairs: max_det %d outside 1..%d", max_det, kRows);
    const size_t enc_bytes = (size_t)kChunk * kRows * (kTrk + kK1) * sizeof(float) + kChunk * kCnt * sizeof(int32_t);
    if (ctx->tracking_enc.reserve(enc_bytes) != DODT_OK) return DODT_ERR_HIP;
    float* trk = static_cast<float*>(ctx->tracking_enc.ptr);
    float* k1 = trk + (size_t)kChunk * kRows * kTrk;
    int32_t* cnt = reinterpret_cast<int32_t*>(k1 + (size_t)kChunk * kRows * kK1);
    const size_t rec_bytes = records_f64 ? sizeof(double) : sizeof(float);
    for (int p0 = 0; p0 < n_pairs; p0 += kChunk) {
        const int n = n_pairs - p0 < kChunk ? n_pairs - p0 : kChunk;
        const char* rec = static_cast<const char*>(d_records) + (size_t)p0 * 2 * max_det * kRecCols * rec_bytes;
        int rc = encode(ctx, rec, records_f64, d_counts + 2 * p0, n, max_det, p2, image_w, image_h, score_threshold,
                        trk, k1, cnt);
        if (rc != DODT_OK) return rc;
        rc = walk(ctx, d_state, Lists{trk, k1, cnt, kCnt, kRows}, n, high_threshold, iou_threshold, t_min);
        if (rc != DODT_OK) return rc;
    }
    return DODT_OK;
}

extern "C" int dodt_track_lanes_stride(int log_capacity, size_t* stride) {
    DODT_REQUIRE(log_capacity >= 1 && stride, "dodt_track_lanes_stride: bad arguments");
    *stride = (state_bytes(log_capacity) + 255) / 256 * 256;
    return DODT_OK;
}

extern "C" int dodt_track_lanes(dodt_ctx* ctx, void* d_states, size_t stride, int n_lanes,
                                const unsigned char* active, const void* d_records, int records_f64,
                                const int32_t* d_counts, int max_det, const double* p2s, const double* image_whs,
                                double score_threshold, double high_threshold, double iou_threshold, int t_min) {
    DODT_REQUIRE(ctx && d_states && n_lanes >= 0, "dodt_track_lanes: bad arguments");
    if (n_lanes == 0) return DODT_OK;
    DODT_REQUIRE(d_records && d_counts && p2s && image_whs, "dodt_track_lanes: NULL argument");
    DODT_REQUIRE(max_det >= 1 && max_det <= kRows, "dodt_track_lanes: max_det %d outside 1..%d", max_det, kRows);
    DODT_REQUIRE(stride >= state_bytes(1) && stride % alignof(Header) == 0,
                 "dodt_track_lanes: stride %zu is no distance between two states", stride);
    const size_t enc_bytes = (size_t)kChunk * kRows * (kTrk + kK1) * sizeof(float) + kChunk * kCnt * sizeof(int32_t);
    if (ctx->tracking_enc.reserve(enc_bytes) != DODT_OK) return DODT_ERR_HIP;
    if (ctx->tracking_ws.reserve((size_t)kChunk * (kCols + kRows) * kCols * sizeof(double)) != DODT_OK)
        return DODT_ERR_HIP;
    float* trk = static_cast<float*>(ctx->tracking_enc.ptr);
    float* k1 = trk + (size_t)kChunk * kRows * kTrk;
    int32_t* cnt = reinterpret_cast<int32_t*>(k1 + (size_t)kChunk * kRows * kK1);
    double* T = static_cast<double*>(ctx->tracking_ws.ptr);
    double* S = T + (size_t)kChunk * kCols * kCols;
    const Lists ls{trk, k1, cnt, kCnt, kRows};
    const size_t rec_bytes = records_f64 ? sizeof(double) : sizeof(float);
    for (int l0 = 0; l0 < n_lanes; l0 += kChunk) {
        const int n = n_lanes - l0 < kChunk ? n_lanes - l0 : kChunk;
        LaneTable tab{};
        unsigned mask = 0;
        for (int i = 0; i < n; ++i) {
            memcpy(tab.c[i].P.p, p2s + (size_t)(l0 + i) * 12, sizeof(tab.c[i].P.p));
            tab.c[i].iw = image_whs[2 * (l0 + i)];
            tab.c[i].ih = image_whs[2 * (l0 + i) + 1];
            if (!active || active[l0 + i]) mask |= 1u << i;
        }
        if (!mask) continue;
        const char* rec = static_cast<const char*>(d_records) + (size_t)l0 * 2 * max_det * kRecCols * rec_bytes;
        char* states = static_cast<char*>(d_states) + (size_t)l0 * stride;
        if (records_f64)
            hipLaunchKernelGGL((encode_lanes_kernel<double, kChunk>), dim3(n), dim3(kThreads), 0, ctx->stream,
                               reinterpret_cast<const double*>(rec), d_counts + 2 * l0, max_det, tab, mask,
                               score_threshold, trk, k1, cnt);
        else
            hipLaunchKernelGGL((encode_lanes_kernel<float, kChunk>), dim3(n), dim3(kThreads), 0, ctx->stream,
                               reinterpret_cast<const float*>(rec), d_counts + 2 * l0, max_det, tab, mask,
                               score_threshold, trk, k1, cnt);
        DODT_LAUNCH_CHECK();
        hipLaunchKernelGGL(iou_tables_lanes_kernel, dim3(kCols + kRows, n), dim3(kThreads), 0, ctx->stream, ls, mask,
                           static_cast<const char*>(states), stride, T, S);
        DODT_LAUNCH_CHECK();
        hipLaunchKernelGGL(walk_lanes_kernel, dim3(n), dim3(kThreads), 0, ctx->stream, ls, mask, states, stride, T, S,
                           iou_threshold, (float)high_threshold, t_min);
        DODT_LAUNCH_CHECK();
    }
    return DODT_OK;
}

extern "C" int dodt_track_encoded(dodt_ctx* ctx, void* d_state, const float* d_track, const float* d_ious,
                                  const int32_t* d_counts, int n_pairs, int max_rows, double high_threshold,
                                  double iou_threshold, int t_min) {
    DODT_REQUIRE(ctx && d_state && n_pairs >= 0, "dodt_track_encoded: bad arguments");
    if (n_pairs == 0) return DODT_OK;
    DODT_REQUIRE(d_track && d_ious && d_counts, "dodt_track_encoded: NULL argument");
    DODT_REQUIRE(max_rows >= 1 && max_rows <= kRows, "dodt_track_encoded: max_rows %d outside 1..%d", max_rows, kRows);
    for (int p0 = 0; p0 < n_pairs; p0 += kChunk) {
        const int n = n_pairs - p0 < kChunk ? n_pairs - p0 : kChunk;
        const Lists ls{d_track + (size_t)p0 * max_rows * kTrk, d_ious + (size_t)p0 * max_rows * kK1, d_counts + 2 * p0,
                       2, max_rows};
        const int rc = walk(ctx, d_state, ls, n, high_threshold, iou_threshold, t_min);
        if (rc != DODT_OK) return rc;
    }
    return DODT_OK;
}
