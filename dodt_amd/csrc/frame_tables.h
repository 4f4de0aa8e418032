// Per-frame skip tables of the fp32 pyramid BEV net, built on the device (dodt_extractor_set_frame_tables).
//
// The static skip tables (dodt_extractor_set_input_support) know the calibration only.  Inside the camera's wedge a
// frame's BEV map is mostly empty too, so each forward filters every layer's static table once more by the cells that
// are non-zero in THIS frame's input.  The rule is the static tables' geometry at cell resolution, on bit masks
// (bit x & 31 of word x >> 5 of a row): 3x3 convs dilate by 1, pools OR 2x2 windows, transposed convs dilate the 2x
// nearest upsampling by 2, concat ORs; an item is kept if the mask has a bit inside the outputs it writes.
//
// The rule is written once, for the host and the device: a "team" of nthr threads (tid 0 of 1 on the host) walks the
// words of a phase with that stride and meets at sync() between phases.  On the device one workgroup per frame holds
// the two working masks in LDS (conv_skip.hip frame_walk_kernel); the host entry dodt_frame_tables_host runs the same
// functions on vectors.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace dodt {
namespace ft {

#define DODT_FT_HD __host__ __device__ inline

constexpr int kLayers = 16;   // the pyramid net's layers in launch order (extractor.h LayerId, which asserts the count)
constexpr int kTables = 2 * kLayers;   // a layer's main and tail launch
// the decoder behind the ten convs alternates transposed conv and fusion conv (walk() below; extractor.h asserts that
// these are the net's upconv layers)
constexpr bool transposed(int layer) { return layer >= 10 && layer % 2 == 0; }

// one launch's tables
struct Table {
    const int4* items = nullptr;   // the table the frame filters: {frame, channel tile, y0, x0} (nullptr: no such launch)
    int n = 0;
    int th = 0, tw = 0;            // the rectangle of layer outputs an item writes: th x tw from (f y0, f x0), f = 2 for
    int f = 1;                     // a transposed conv (th, tw at the output resolution)
    uint8_t* now = nullptr;        // [n] 1: the item's outputs may depend on this forward's input
    uint8_t* prev = nullptr;       // [n] the same for the last forward into the same buffer
    int4* run = nullptr;           // [n] compacted: the items with now, in the table's order (the launch computes them)
    int* count = nullptr;          // how many
    int4* restore = nullptr;       // [n] compacted: the items with prev and not now, in the table's order (their outputs
    int* rcount = nullptr;         // go back to the input-independent values by copy); how many
};

struct Plan {
    int H = 0, W = 0;              // padded input; level l is (H >> l) x (W >> l)
    int frames = 0;
    uint32_t* stash = nullptr;     // per frame: conv1_2's, conv2_2's and conv3_3's masks until the fusion layers OR them
    Table t[kTables];              // [2 * layer + (tail ? 1 : 0)]
};

DODT_FT_HD int pitch(int w) { return (w + 31) >> 5; }
DODT_FT_HD int level_words(int H, int W, int l) { return (H >> l) * pitch(W >> l); }
DODT_FT_HD int stash_words(int H, int W) { return level_words(H, W, 0) + level_words(H, W, 1) + level_words(H, W, 2); }

// the bits of a row's last word that lie inside the row
DODT_FT_HD uint32_t last_mask(int w) { return (w & 31) ? (1u << (w & 31)) - 1u : 0xffffffffu; }

// dst = src dilated by r along x (r <= 2)
template <class Sync>
DODT_FT_HD void hdilate(uint32_t* dst, const uint32_t* src, int h, int w, int r, int tid, int nthr, Sync sync) {
    const int p = pitch(w), n = h * p;
    for (int i = tid; i < n; i += nthr) {
        const int k = i % p;
        const uint32_t c = src[i], lo = k > 0 ? src[i - 1] : 0u, hi = k < p - 1 ? src[i + 1] : 0u;
        uint32_t o = c;
        for (int d = 1; d <= r; ++d) o |= (c << d) | (lo >> (32 - d)) | (c >> d) | (hi << (32 - d));
        if (k == p - 1) o &= last_mask(w);
        dst[i] = o;
    }
    sync();
}

// dst = src dilated by r along y
template <class Sync>
DODT_FT_HD void vdilate(uint32_t* dst, const uint32_t* src, int h, int w, int r, int tid, int nthr, Sync sync) {
    const int p = pitch(w), n = h * p;
    for (int i = tid; i < n; i += nthr) {
        const int y = i / p;
        uint32_t o = 0;
        for (int d = -r; d <= r; ++d)
            if (y + d >= 0 && y + d < h) o |= src[i + d * p];
        dst[i] = o;
    }
    sync();
}

// cur = cur dilated by r in both directions (tmp: as large as cur)
template <class Sync>
DODT_FT_HD void dilate(uint32_t* cur, uint32_t* tmp, int h, int w, int r, int tid, int nthr, Sync sync) {
    hdilate(tmp, cur, h, w, r, tid, nthr, sync);
    vdilate(cur, tmp, h, w, r, tid, nthr, sync);
}

// the even bits of v | v >> 1, packed into the low half
DODT_FT_HD uint32_t squash_pairs(uint32_t v) {
    v = (v | (v >> 1)) & 0x55555555u;
    v = (v | (v >> 1)) & 0x33333333u;
    v = (v | (v >> 2)) & 0x0f0f0f0fu;
    v = (v | (v >> 4)) & 0x00ff00ffu;
    v = (v | (v >> 8)) & 0x0000ffffu;
    return v;
}

// the low 16 bits of v, each one twice
DODT_FT_HD uint32_t spread_pairs(uint32_t v) {
    v &= 0xffffu;
    v = (v | (v << 8)) & 0x00ff00ffu;
    v = (v | (v << 4)) & 0x0f0f0f0fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v | (v << 1);
}

// dst (h / 2 x w / 2) = VALID 2x2 pool of src (h x w)
template <class Sync>
DODT_FT_HD void pool2(uint32_t* dst, const uint32_t* src, int h, int w, int tid, int nthr, Sync sync) {
    const int sp = pitch(w), dh = h / 2, dw = w / 2, dp = pitch(dw), n = dh * dp;
    for (int i = tid; i < n; i += nthr) {
        const int y = i / dp, k = i - y * dp;
        const uint32_t* r0 = src + (2 * y) * sp;
        const uint32_t* r1 = r0 + sp;
        const uint32_t a = r0[2 * k] | r1[2 * k];
        const uint32_t b = 2 * k + 1 < sp ? (r0[2 * k + 1] | r1[2 * k + 1]) : 0u;
        uint32_t o = squash_pairs(a) | (squash_pairs(b) << 16);
        if (k == dp - 1) o &= last_mask(dw);
        dst[i] = o;
    }
    sync();
}

// dst (2h x 2w) = nearest 2x upsampling of src (h x w)
template <class Sync>
DODT_FT_HD void expand2(uint32_t* dst, const uint32_t* src, int h, int w, int tid, int nthr, Sync sync) {
    const int sp = pitch(w), dp = pitch(2 * w), n = 2 * h * dp;
    for (int i = tid; i < n; i += nthr) {
        const int y = i / dp, k = i - y * dp;
        dst[i] = spread_pairs(src[(y >> 1) * sp + (k >> 1)] >> (16 * (k & 1)));
    }
    sync();
}

template <class Sync>
DODT_FT_HD void copy_words(uint32_t* dst, const uint32_t* src, int n, int tid, int nthr, Sync sync) {
    for (int i = tid; i < n; i += nthr) dst[i] = src[i];
    sync();
}

template <class Sync>
DODT_FT_HD void or_words(uint32_t* dst, const uint32_t* src, int n, int tid, int nthr, Sync sync) {
    for (int i = tid; i < n; i += nthr) dst[i] |= src[i];
    sync();
}

// does [y0, y1) x [x0, x1), clipped to the map, hold a bit?
DODT_FT_HD bool any_bit(const uint32_t* m, int h, int w, int y0, int y1, int x0, int x1) {
    if (y0 < 0) y0 = 0;
    if (x0 < 0) x0 = 0;
    if (y1 > h) y1 = h;
    if (x1 > w) x1 = w;
    if (y0 >= y1 || x0 >= x1) return false;
    const int p = pitch(w), k0 = x0 >> 5, k1 = (x1 - 1) >> 5;
    const uint32_t first = 0xffffffffu << (x0 & 31), last = 0xffffffffu >> (31 - ((x1 - 1) & 31));
    uint32_t acc = 0;
    for (int y = y0; y < y1; ++y) {
        const uint32_t* row = m + y * p;
        for (int k = k0; k <= k1; ++k) {
            uint32_t v = row[k];
            if (k == k0) v &= first;
            if (k == k1) v &= last;
            acc |= v;
        }
    }
    return acc != 0;
}

// the items of `frame` in a layer's tables against the layer's mask (h x w: the layer's outputs)
template <class Sync>
DODT_FT_HD void mark(const Plan& pl, int layer, int frame, const uint32_t* m, int h, int w, int tid, int nthr, Sync sync) {
    for (int j = 0; j < 2; ++j) {
        const Table& t = pl.t[2 * layer + j];
        if (!t.items) continue;
        for (int i = tid; i < t.n; i += nthr) {
            const int4 it = t.items[i];
            if (it.x != frame) continue;
            t.now[i] = any_bit(m, h, w, t.f * it.z, t.f * it.z + t.th, t.f * it.w, t.f * it.w + t.tw) ? 1 : 0;
        }
    }
    sync();
}

// One frame through the net.  a, b: working masks of level_words(H, W, 0) words each; a holds the frame's non-zero
// input cells (bits beyond a row's end clear).  Layers in launch order: conv1_1, conv1_2, conv2_1, conv2_2, conv3_1,
// conv3_2, conv3_3, conv4_1, conv4_2, conv4_3, upconv3, pyramid_fusion3, upconv2, pyramid_fusion2, upconv1,
// pyramid_fusion1.
template <class Sync>
DODT_FT_HD void walk(const Plan& pl, int frame, uint32_t* a, uint32_t* b, int tid, int nthr, Sync sync) {
    uint32_t* cur = a;
    uint32_t* tmp = b;
    auto swap = [&]() { uint32_t* s = cur; cur = tmp; tmp = s; };
    uint32_t* stash[3];
    stash[0] = pl.stash + (size_t)frame * stash_words(pl.H, pl.W);
    stash[1] = stash[0] + level_words(pl.H, pl.W, 0);
    stash[2] = stash[1] + level_words(pl.H, pl.W, 1);
    int layer = 0;
    const int convs[4] = {2, 2, 3, 3};
    for (int l = 0; l < 4; ++l) {
        const int h = pl.H >> l, w = pl.W >> l;
        for (int c = 0; c < convs[l]; ++c) {
            dilate(cur, tmp, h, w, 1, tid, nthr, sync);
            mark(pl, layer++, frame, cur, h, w, tid, nthr, sync);
        }
        if (l < 3) {
            copy_words(stash[l], cur, level_words(pl.H, pl.W, l), tid, nthr, sync);
            pool2(tmp, cur, h, w, tid, nthr, sync);
            swap();
        }
    }
    for (int l = 2; l >= 0; --l) {
        const int h = pl.H >> l, w = pl.W >> l;
        expand2(tmp, cur, h / 2, w / 2, tid, nthr, sync);
        swap();
        dilate(cur, tmp, h, w, 2, tid, nthr, sync);
        mark(pl, layer++, frame, cur, h, w, tid, nthr, sync);         // upconv
        or_words(cur, stash[l], level_words(pl.H, pl.W, l), tid, nthr, sync);   // concat
        dilate(cur, tmp, h, w, 1, tid, nthr, sync);
        mark(pl, layer++, frame, cur, h, w, tid, nthr, sync);         // pyramid_fusion
    }
}

// Compaction of one table by a team into two lists, both in the table's order: run = the items with now (count of
// them), restore = the items with prev and not now (rcount), and prev = now for the next forward.  scan: [nthr + 1]
// ints the team shares (a kept item adds 1, a restored one 1 << 16: both prefix sums in one scan; nthr <= 32768).
// prev: the table's own or, for the layer that writes the caller's buffers, that buffer pair's.
template <class Sync>
DODT_FT_HD void compact(const Table& t, uint8_t* prev, int* scan, int tid, int nthr, Sync sync) {
    int base = 0, rbase = 0;
    for (int i0 = 0; i0 < t.n; i0 += nthr) {
        const int i = i0 + tid;
        const uint8_t now = i < t.n ? t.now[i] : 0;
        const int keep = i < t.n && now ? 1 : 0;
        const int back = i < t.n && !now && prev[i] ? 1 : 0;
        if (i < t.n) prev[i] = now;
        scan[tid + 1] = keep | (back << 16);
        if (tid == 0) scan[0] = 0;
        sync();
        for (int d = 1; d < nthr; d <<= 1) {      // inclusive scan of scan[1 .. nthr]
            const int v = tid + 1 > d ? scan[tid + 1 - d] : 0;
            sync();
            scan[tid + 1] += v;
            sync();
        }
        if (keep) t.run[base + (scan[tid] & 0xffff)] = t.items[i];
        if (back) t.restore[rbase + (scan[tid] >> 16)] = t.items[i];
        base += scan[nthr] & 0xffff;
        rbase += scan[nthr] >> 16;
        sync();
    }
    if (tid == 0) {
        *t.count = base;
        *t.rcount = rbase;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Restoring: the outputs of a table's restore items go back to the constants store's values by copy
// ---------------------------------------------------------------------------------------------------------------
// one table's restore list and where its items' outputs live
struct RestoreTable {
    const int4* list = nullptr;    // {frame, channel tile, y0, x0} (nullptr: no such launch)
    const int* count = nullptr;
    float* dst = nullptr;          // the live CB8 map; nullptr: the caller's NHWC pair (pyramid_fusion1)
    const float* src = nullptr;    // the store's map (one frame)
    long long frame_stride = 0;    // of dst, floats
    int H = 0, W = 0;              // the map's size
    int ch0 = 0, bn = 0;           // channel tile n holds channels ch0 + n bn ..
    int f = 1, th = 0, tw = 0;     // an item writes th x tw outputs from (f y0, f x0)
    float* pool_dst = nullptr;     // the fused 2x2 pool's map (channel tile n: channels n bn ..), or nullptr
    const float* pool_src = nullptr;
    long long pool_frame_stride = 0;
};
struct RestorePlan {
    RestoreTable t[kTables];
    const float* feat = nullptr;   // the store's (feature, bottleneck) pair, one frame, pad rows sliced off
    const float* bneck = nullptr;
    int pad_top = 0, out_h = 0, out_c = 0;
};

struct alignas(16) Quad { float v[4]; };   // 16 bytes per load and store

// th x tw cells of nch channels from (y0, x0) of a CB8 map ([C / 8][H][W][8]), clipped to the map
DODT_FT_HD void restore_cb8(float* dst, const float* src, int H, int W, int ch0, int nch, int y0, int x0, int th, int tw,
                            int tid, int nthr) {
    const int tw2 = tw * 2, per_plane = th * tw2, n = (nch >> 3) * per_plane;
    const Quad* s4 = reinterpret_cast<const Quad*>(src);
    Quad* d4 = reinterpret_cast<Quad*>(dst);
    for (int i = tid; i < n; i += nthr) {
        const int p = i / per_plane, r = (i - p * per_plane) / tw2, c = i - p * per_plane - r * tw2;
        const int y = y0 + r, x2 = x0 * 2 + c;
        if (y >= H || x2 >= W * 2) continue;
        const size_t off = ((size_t)((ch0 >> 3) + p) * H + y) * (W * 2) + x2;
        d4[off] = s4[off];
    }
}

// One restore item by a team.  A layer buffer: the tile's channels and, where the pool is fused, the pooled tile.
// pyramid_fusion1 (t.dst == nullptr): the rows of the caller's NHWC feature map (row pad_top of the layer's grid is its
// row 0) and, for channel tile 0, the same cells of the bottleneck map.
DODT_FT_HD void restore_item(const RestorePlan& pl, const RestoreTable& t, int4 it, float* feat, float* bneck, int tid,
                             int nthr) {
    const int y0 = t.f * it.z, x0 = t.f * it.w;
    if (t.dst) {
        restore_cb8(t.dst + (size_t)it.x * t.frame_stride, t.src, t.H, t.W, t.ch0 + it.y * t.bn, t.bn, y0, x0, t.th, t.tw,
                    tid, nthr);
        if (t.pool_dst)
            restore_cb8(t.pool_dst + (size_t)it.x * t.pool_frame_stride, t.pool_src, t.H >> 1, t.W >> 1, it.y * t.bn, t.bn,
                        y0 >> 1, x0 >> 1, t.th >> 1, t.tw >> 1, tid, nthr);
        return;
    }
    const int c4n = t.bn >> 2, row4 = t.W * (pl.out_c >> 2), n = t.th * t.tw * c4n;
    const Quad* s4 = reinterpret_cast<const Quad*>(pl.feat);
    Quad* d4 = reinterpret_cast<Quad*>(feat) + (size_t)it.x * pl.out_h * row4;
    for (int j = tid; j < n; j += nthr) {
        const int r = j / (t.tw * c4n), x = (j - r * t.tw * c4n) / c4n, c = j - (r * t.tw + x) * c4n;
        const int y = y0 + r - pl.pad_top;
        if (y < 0 || y >= pl.out_h || x0 + x >= t.W) continue;
        const size_t off = (size_t)y * row4 + (size_t)(x0 + x) * (pl.out_c >> 2) + ((t.ch0 + it.y * t.bn) >> 2) + c;
        d4[off] = s4[off];
    }
    if (bneck && pl.bneck && it.y == 0) {
        const int tw4 = t.tw >> 2, w4 = t.W >> 2;
        const Quad* b4 = reinterpret_cast<const Quad*>(pl.bneck);
        Quad* o4 = reinterpret_cast<Quad*>(bneck) + (size_t)it.x * pl.out_h * w4;
        for (int j = tid; j < t.th * tw4; j += nthr) {
            const int r = j / tw4, c = (x0 >> 2) + j - r * tw4;
            const int y = y0 + r - pl.pad_top;
            if (y < 0 || y >= pl.out_h || c >= w4) continue;
            o4[(size_t)y * w4 + c] = b4[(size_t)y * w4 + c];
        }
    }
}

#undef DODT_FT_HD

}  // namespace ft
}  // namespace dodt
