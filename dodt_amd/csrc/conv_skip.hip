// Skip machinery of the fp32 pyramid extractor: the static skip tables (dodt_extractor_set_input_support), the
// per-frame tables built on the device (dodt_extractor_set_frame_tables, frame_tables.h), the constants store the
// stale tiles are restored from, the choice of table per launch, and what the work accounting reads of all that.
#include <algorithm>
#include <cstring>

#include "conv_variants.h"
#include "extractor.h"

using namespace dodt;
using dodt::ft::RestoreTable;
using dodt::ft::RestorePlan;

namespace {

// ---------------------------------------------------------------------------
// input support: where a layer's outputs can depend on the input (dodt_extractor_set_input_support)
// ---------------------------------------------------------------------------
// An output whose receptive field holds only inputs that are zero in every frame (zero padding included) is a
// function of the weights alone: a full forward writes it, and later forwards need not.
struct Support {
    int h = 0, w = 0;
    std::vector<uint8_t> m;   // 1: may depend on the input
    Support() = default;
    Support(int h_, int w_) : h(h_), w(w_), m((size_t)h_ * w_, 0) {}
    uint8_t& at(int y, int x) { return m[(size_t)y * w + x]; }
    uint8_t at(int y, int x) const { return m[(size_t)y * w + x]; }
};

// the outputs of a 3x3 SAME conv (r = 1), or the margin of a transposed conv (r = 2)
Support dilate(const Support& a, int r) {
    Support t(a.h, a.w), o(a.h, a.w);
    for (int y = 0; y < a.h; ++y)
        for (int x = 0; x < a.w; ++x)
            for (int d = -r; d <= r; ++d)
                if (x + d >= 0 && x + d < a.w && a.at(y, x + d)) { t.at(y, x) = 1; break; }
    for (int y = 0; y < a.h; ++y)
        for (int x = 0; x < a.w; ++x)
            for (int d = -r; d <= r; ++d)
                if (y + d >= 0 && y + d < a.h && t.at(y + d, x)) { o.at(y, x) = 1; break; }
    return o;
}

// VALID 2x2 max pool (odd sizes floored)
Support pool2(const Support& a) {
    Support o(a.h / 2, a.w / 2);
    for (int y = 0; y < o.h; ++y)
        for (int x = 0; x < o.w; ++x)
            o.at(y, x) = a.at(2 * y, 2 * x) | a.at(2 * y, 2 * x + 1) | a.at(2 * y + 1, 2 * x) | a.at(2 * y + 1, 2 * x + 1);
    return o;
}

// 3x3 stride-2 transposed conv: input i reaches outputs 2i .. 2i + 2 (or 2i - 1 .. 2i + 1 for the other padding
// split); nearest 2x upsampling dilated by 2 covers both
Support upconv2(const Support& a) {
    Support u(2 * a.h, 2 * a.w);
    for (int y = 0; y < u.h; ++y)
        for (int x = 0; x < u.w; ++x) u.at(y, x) = a.at(y / 2, x / 2);
    return dilate(u, 2);
}

// summed-area table: does a rectangle hold an input-dependent output?
struct SupportSum {
    int h = 0, w = 0;
    std::vector<int> s;
    explicit SupportSum(const Support& a) : h(a.h), w(a.w), s((size_t)(a.h + 1) * (a.w + 1), 0) {
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                s[(size_t)(y + 1) * (w + 1) + x + 1] = a.at(y, x) + s[(size_t)y * (w + 1) + x + 1] +
                                                       s[(size_t)(y + 1) * (w + 1) + x] - s[(size_t)y * (w + 1) + x];
    }
    bool any(int y0, int y1, int x0, int x1) const {   // [y0, y1) x [x0, x1), clipped
        y0 = std::max(y0, 0); x0 = std::max(x0, 0); y1 = std::min(y1, h); x1 = std::min(x1, w);
        if (y0 >= y1 || x0 >= x1) return false;
        return s[(size_t)y1 * (w + 1) + x1] - s[(size_t)y0 * (w + 1) + x1] - s[(size_t)y1 * (w + 1) + x0] +
                   s[(size_t)y0 * (w + 1) + x0] > 0;
    }
};

// Winograd F(4x4,3x3): an output's fp32 value depends on the whole 6 x 6 input tile of its 4 x 4 block (the
// transforms are dense: taps outside its 3 x 3 field cancel exactly, not in rounding).  (F(2x2,3x3) has no such
// reach: output 0 of a block never reads input 3, output 1 never input 0.)
Support wino_blocks(const Support& a, int m) {
    const SupportSum sum(a);
    Support o(a.h, a.w);
    for (int y0 = 0; y0 < a.h; y0 += m)
        for (int x0 = 0; x0 < a.w; x0 += m)
            if (sum.any(y0 - 1, y0 + m + 1, x0 - 1, x0 + m + 1))
                for (int y = y0; y < std::min(y0 + m, a.h); ++y)
                    for (int x = x0; x < std::min(x0 + m, a.w); ++x) o.at(y, x) = 1;
    return o;
}

// ---------------------------------------------------------------------------
// per-frame tables (frame_tables.h): three launches at the head of a forward
// ---------------------------------------------------------------------------
// the non-zero cells of the frames' input maps (NHWC, any channel) as bit masks: half a wave per word.  A cell that
// holds only -0.0 counts as empty (the sign bit is masked off): every conv form starts its accumulators at +0.0 and
// x w with x = -0.0 adds +-0.0, so its outputs are bit for bit those of +0.0, the value the skipped outputs were
// computed from (tests/test_gpu_bev_skip_adversarial.py).  A denormal counts as non-zero.
__global__ void __launch_bounds__(256)
frame_support_kernel(const float* __restrict__ x, long long frame_stride, int H, int W, int C, uint32_t* __restrict__ bits) {
    const int p = dodt::ft::pitch(W), words = H * p;
    const int word = blockIdx.x * 8 + (threadIdx.x >> 5), frame = blockIdx.y;
    const int y = word / p, cx = (word - y * p) * 32 + (threadIdx.x & 31);
    bool nz = false;
    if (word < words && cx < W) {
        const uint2* c = reinterpret_cast<const uint2*>(x + (size_t)frame * frame_stride + ((size_t)y * W + cx) * C);
        uint32_t acc = 0;
        for (int k = 0; k < C / 2; ++k) {      // (C is even: dodt_extractor_create)
            const uint2 v = c[k];
            acc |= v.x | v.y;
        }
        nz = (acc & 0x7fffffffu) != 0;
    }
    const unsigned long long b = __ballot(nz);
    if ((threadIdx.x & 31) == 0 && word < words)
        bits[(size_t)frame * words + word] = (uint32_t)((threadIdx.x & 32) ? b >> 32 : b);
}

// one workgroup per frame walks the net's geometry on two masks in LDS and marks the items its frame reaches
__global__ void __launch_bounds__(1024)
frame_walk_kernel(const dodt::ft::Plan* __restrict__ pl, const uint32_t* __restrict__ bits) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ft_lds[];
    const int words = dodt::ft::level_words(pl->H, pl->W, 0);
    uint32_t* a = ft_lds;
    uint32_t* b = ft_lds + words;
    const int frame = blockIdx.x;
    for (int i = threadIdx.x; i < words; i += blockDim.x) a[i] = bits[(size_t)frame * words + i];
    __syncthreads();
    dodt::ft::walk(*pl, frame, a, b, (int)threadIdx.x, (int)blockDim.x, [] { __syncthreads(); });
}

// one workgroup per table: the items this forward runs, in the table's order (a prefix sum: the same table for the
// same masks, whatever order the workgroups run in)
__global__ void __launch_bounds__(256)
frame_compact_kernel(const dodt::ft::Plan* __restrict__ pl, uint8_t* last_prev_main, uint8_t* last_prev_tail) {
    __shared__ int scan[257];
    const dodt::ft::Table t = pl->t[blockIdx.x];
    if (!t.items) return;
    const bool last = (int)blockIdx.x / 2 == dodt::ft::kLayers - 1;     // pyramid_fusion1: the output pair's set
    uint8_t* prev = last ? ((blockIdx.x & 1) ? last_prev_tail : last_prev_main) : t.prev;
    dodt::ft::compact(t, prev, scan, (int)threadIdx.x, (int)blockDim.x, [] { __syncthreads(); });
}

// Every table's restore list in one launch (ahead of conv1_1 on the extractor's stream): the outputs of an item that
// the last forward into the same buffer reached and this one does not go back to the store's values.  Workgroups
// stride over the lists end to end; one that finds nothing leaves at once.  last_on: pyramid_fusion1's list counts
// (the output pair is one the layer remembers).
__global__ void __launch_bounds__(256)
frame_restore_kernel(const RestorePlan* __restrict__ pl, float* __restrict__ feat, float* __restrict__ bneck, int last_on) {
    __shared__ int start[dodt::ft::kTables + 1];
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int k = 0; k < dodt::ft::kTables; ++k) {
            start[k] = sum;
            const bool on = pl->t[k].list && (k / 2 != dodt::ft::kLayers - 1 || last_on);
            sum += on ? *pl->t[k].count : 0;
        }
        start[dodt::ft::kTables] = sum;
    }
    __syncthreads();
    const int total = start[dodt::ft::kTables];
    int k = 0;
    for (int i = blockIdx.x; i < total; i += gridDim.x) {
        while (i >= start[k + 1]) ++k;
        dodt::ft::restore_item(*pl, pl->t[k], pl->t[k].list[i - start[k]], feat, bneck, (int)threadIdx.x, (int)blockDim.x);
    }
}

void free_store(dodt_extractor* ex) {
    for (int i = 0; i < NBUF; ++i) {
        if (ex->store[i]) (void)hipFree(ex->store[i]);
        ex->store[i] = nullptr;
    }
    if (ex->store_feat) (void)hipFree(ex->store_feat);
    if (ex->store_bneck) (void)hipFree(ex->store_bneck);
    if (ex->d_restore_plan) (void)hipFree(ex->d_restore_plan);
    ex->store_feat = ex->store_bneck = nullptr;
    ex->d_restore_plan = nullptr;
    ex->store_valid = false;
    ex->store_bytes = 0;
}

// the builder's launches for the pass's input; slot: the output pair's item set of pyramid_fusion1
int build_frame_tables(const dodt_extractor* ex, const Pass& p, int slot) {
    const Buffer& x0 = ex->buf[X0];
    const int words = ft::level_words(ex->H, ex->W, 0);
    hipStream_t s = ex->ctx->stream;
    hipLaunchKernelGGL(frame_support_kernel, dim3((unsigned)ceil_div(words, 8), (unsigned)p.frames), dim3(256), 0, s,
                       p.map[X0], (long long)x0.frame_floats(), ex->H, ex->W, x0.C, ex->d_frame_bits);
    DODT_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_walk_kernel, dim3((unsigned)p.frames), dim3(1024), (size_t)words * 8, s,
                       ex->d_frame_plan, ex->d_frame_bits);
    DODT_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_compact_kernel, dim3(ft::kTables), dim3(256), 0, s, ex->d_frame_plan,
                       ex->out_prev[slot][0], ex->out_prev[slot][1]);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

void free_skip_tables(dodt_extractor* ex) {
    free_frame_tables(ex);     // (they filter the skip tables)
    for (Layer& l : ex->layers) {
        for (Launch* ln : {&l.main, &l.tail}) {
            if (ln->d_skip) (void)hipFree(ln->d_skip);
            ln->d_skip = nullptr;
            ln->n_skip = -1;
        }
        l.skip_frac = 1.0;
    }
    ex->skip_on = false;
}

// device allocations that live as long as a function call
struct Temps {
    std::vector<void*> ptrs;
    ~Temps() { for (void* p : ptrs) (void)hipFree(p); }
    hipError_t alloc(void** p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
};

// The constants store: frame 0 of a forward on a zero input, through the same kernels and the full tables, written into
// the store's maps in place of the layer buffers: a pass of its own, so neither the caller's input, a live buffer nor
// the extractor's state beside the store is touched.  Waits for the stream (once per weight load).
int take_store(dodt_extractor* ex) {
    hipStream_t s = ex->ctx->stream;
    if (!ex->d_restore_plan) {
        size_t total = 0;
        hipError_t ea = hipSuccess;
        for (int i = 0; i < NBUF && ea == hipSuccess; ++i) {
            if (i == X0 || i == F1 || !ex->buf[i].ptr) continue;
            const size_t bytes = ex->buf[i].frame_floats() * sizeof(float);
            ea = hipMalloc(&ex->store[i], bytes);
            total += bytes;
        }
        const size_t px = (size_t)ex->out_h * ex->out_w;
        if (ea == hipSuccess) ea = hipMalloc(&ex->store_feat, px * ex->out_c * sizeof(float));
        if (ea == hipSuccess) ea = hipMalloc(&ex->store_bneck, px * sizeof(float));
        if (ea == hipSuccess) ea = hipMalloc(&ex->d_restore_plan, sizeof(RestorePlan));
        if (ea != hipSuccess) free_store(ex);     // (nothing half-allocated stays behind)
        DODT_HIP_CHECK(ea);
        ex->store_bytes = total + px * (ex->out_c + 1) * sizeof(float);
    }
    // the pass: the store's maps, a zero input frame, every full table's items of frame 0, no events
    Temps temps;
    Pass p;
    p.frames = 1;
    for (int i = 0; i < NBUF; ++i) p.map[i] = ex->store[i];
    const size_t in_bytes = ex->buf[X0].frame_floats() * sizeof(float);
    DODT_HIP_CHECK(temps.alloc((void**)&p.map[X0], in_bytes));
    DODT_HIP_CHECK(hipMemsetAsync(p.map[X0], 0, in_bytes, s));
    for (size_t li = 0; li < ex->layers.size(); ++li) {
        const Layer& l = ex->layers[li];
        // a main table lists its items frame by frame (plan_layer): frame 0's are its head.  A tail's are not.
        const std::vector<int4>& mi = l.main.h_items;
        const int n0 = (int)(std::find_if(mi.begin(), mi.end(), [](const int4& it) { return it.x != 0; }) - mi.begin());
        p.table[li][0] = {l.main.d_items, n0, nullptr, true};
        std::vector<int4> first;
        for (const int4& it : l.tail.h_items)
            if (it.x == 0) first.push_back(it);
        if (first.empty()) continue;
        int4* d = nullptr;
        DODT_HIP_CHECK(temps.alloc((void**)&d, first.size() * sizeof(int4)));
        DODT_HIP_CHECK(hipMemcpy(d, first.data(), first.size() * sizeof(int4), hipMemcpyHostToDevice));
        p.table[li][1] = {d, (int)first.size(), nullptr, false};
    }
    DODT_HIP_CHECK(hipMemsetAsync(ex->d_counters, 0, 4096 * sizeof(int), s));
    const int rc = run_layers(ex, p, ex->store_feat, ex->bneck_loaded ? ex->store_bneck : nullptr);
    DODT_HIP_CHECK(hipStreamSynchronize(s));     // (also ahead of freeing the temporaries where a launch failed)
    if (rc) return rc;
    // where each table's items live (the layer buffers never move; the caller's pair comes with the launch)
    RestorePlan pl;
    for (size_t li = 0; li < ex->layers.size(); ++li) {
        const Layer& l = ex->layers[li];
        const int pool_dst = fused_pool_buffer(l);
        int j = 0;
        for (const Launch* ln : {&l.main, &l.tail}) {
            const ft::Table& ft = ex->frame_plan.t[2 * li + j];
            RestoreTable& t = pl.t[2 * li + j++];
            if (!ft.items) continue;
            const Buffer& dst = ex->buf[l.dst];
            t.list = ft.restore;
            t.count = ft.rcount;
            t.dst = dst.ptr;                 // (nullptr: pyramid_fusion1)
            t.src = ex->store[l.dst];
            t.frame_stride = (long long)dst.frame_floats();
            t.H = dst.H; t.W = dst.W;
            t.ch0 = l.dst_coff;
            t.bn = variants()[ln->variant].BN;
            t.f = ft.f; t.th = ft.th; t.tw = ft.tw;
            if (pool_dst >= 0) {
                t.pool_dst = ex->buf[pool_dst].ptr;
                t.pool_src = ex->store[pool_dst];
                t.pool_frame_stride = (long long)ex->buf[pool_dst].frame_floats();
            }
        }
    }
    pl.feat = ex->store_feat;
    pl.bneck = ex->bneck_loaded && bneck_fused(ex->layers.back()) ? ex->store_bneck : nullptr;   // (not fused: a kernel of its own rewrites the map)
    pl.pad_top = ex->pad_top; pl.out_h = ex->out_h; pl.out_c = ex->out_c;
    DODT_HIP_CHECK(hipMemcpy(ex->d_restore_plan, &pl, sizeof(pl), hipMemcpyHostToDevice));
    ex->store_valid = true;
    return DODT_OK;
}

}  // namespace

namespace dodt {

void free_frame_tables(dodt_extractor* ex) {
    free_store(ex);
    for (void* p : ex->frame_allocs) (void)hipFree(p);
    ex->frame_allocs.clear();
    for (Layer& l : ex->layers)
        for (Launch* ln : {&l.main, &l.tail}) {
            ln->d_run = nullptr;
            ln->d_count = nullptr;
        }
    ex->frame_plan = ft::Plan();
    ex->d_frame_plan = nullptr;
    ex->d_frame_bits = nullptr;
    ex->d_frame_counts = nullptr;
    ex->frame_on = false;
}

int find_pair(const dodt_extractor* ex, const float* feat, const float* bneck) {
    for (int k = 0; k < ex->n_pairs; ++k)
        if (ex->pairs[k].feat == feat && ex->pairs[k].bneck == bneck) return k;
    return -1;
}

int slot_for_new_pair(const dodt_extractor* ex) {
    if (ex->n_pairs == kOutPairs) return ex->pairs[0].slot;
    bool used[kOutPairs] = {};
    for (int k = 0; k < ex->n_pairs; ++k) used[ex->pairs[k].slot] = true;
    int slot = 0;
    while (used[slot]) ++slot;
    return slot;
}

void forget_pairs(dodt_extractor* ex) { ex->n_pairs = 0; }

void add_pair(dodt_extractor* ex, const float* feat, const float* bneck, int slot) {
    if (ex->n_pairs == kOutPairs) {      // the oldest leaves (it is primed again when it comes back)
        std::copy(ex->pairs + 1, ex->pairs + kOutPairs, ex->pairs);
        --ex->n_pairs;
    }
    ex->pairs[ex->n_pairs++] = {feat, bneck, slot};
}

void choose_tables(dodt_extractor* ex, bool skip, bool last_skip, Pass& p) {
    for (size_t li = 0; li < ex->layers.size(); ++li) {
        const Layer& l = ex->layers[li];
        // pyramid_fusion1 writes the caller's buffers: it skips only into a pair it has written with full tables
        const bool on = li == (size_t)FUSION1 ? last_skip : skip;
        const Tables kind = !on ? Tables::Full : ex->frame_on ? Tables::PerFrame : Tables::Static;
        ex->ran[li].kind = kind;
        int j = 0;
        for (const Launch* ln : {&l.main, &l.tail}) {
            ItemTable& t = p.table[li][j];
            if (kind == Tables::Full || ln->n_skip < 0) t = {ln->d_items, ln->n_items, nullptr, true};
            else if (kind == Tables::PerFrame && ln->d_run) t = {ln->d_run, ln->n_skip, ln->d_count, false};
            else t = {ln->d_skip, ln->n_skip, nullptr, false};
            ex->ran[li].n[j++] = t.n;
        }
    }
    // per-frame tables: the stale items go back to their values by copy (a forward that primes has nothing to restore)
    ex->restoring = ex->frame_on && skip;
}

// Per-frame tables: every launch runs the items this input reaches; the ones the last forward into the same buffer
// reached and this one does not go back to their input-independent values (frame_restore_kernel, one launch for all
// tables, behind the builder and ahead of conv1_1), and the builder keeps this input's set for the next forward.  A
// forward on full tables (priming; pyramid_fusion1 into a pair it has not written) records its set the same way.
int begin_frame_forward(dodt_extractor* ex, const Pass& p, int slot, bool last_skip, float* d_feat_out,
                        float* d_bottleneck_out) {
    hipStream_t s = ex->ctx->stream;
    int rc;
    if (ex->restoring && !ex->store_valid) {
        if ((rc = take_store(ex))) return rc;
        DODT_HIP_CHECK(hipMemsetAsync(ex->d_counters, 0, 4096 * sizeof(int), s));
    }
    if ((rc = build_frame_tables(ex, p, slot))) return rc;
    if (ex->restoring) {
        hipLaunchKernelGGL(frame_restore_kernel, dim3((unsigned)(4 * ex->ctx->num_cus)), dim3(256), 0, s,
                           ex->d_restore_plan, d_feat_out, d_bottleneck_out, last_skip ? 1 : 0);
        DODT_LAUNCH_CHECK();
    }
    return DODT_OK;
}

// the per-frame counts of the last forward (waits for the stream); have = false: per-frame tables are off
WorkShare::WorkShare(const dodt_extractor* ex) : have(false) {
    if (!ex->frame_on) return;
    if (hipStreamSynchronize(ex->ctx->stream) != hipSuccess) return;
    have = hipMemcpy(counts, ex->d_frame_counts, sizeof(counts), hipMemcpyDeviceToHost) == hipSuccess;
}

// HBM bytes of the restore copies, read from the store and written: the item's outputs, their pooled copy where the
// pool is fused, the bottleneck cells of a pyramid_fusion1 tile where the bottleneck is
double WorkShare::restore_bytes(const dodt_extractor* ex, const Layer& l) const {
    const size_t li = &l - ex->layers.data();
    const bool pooled = fused_pool_buffer(l) >= 0;
    const bool bneck = &l == &ex->layers.back() && ex->bneck_loaded && bneck_fused(l);
    double b = 0.0;
    int j = 0;
    for (const Launch* ln : {&l.main, &l.tail}) {
        const int jj = j++;
        if (ln->h_items.empty()) continue;
        const KernelVariant& v = variants()[ln->variant];
        const double px = (l.deconv ? 4.0 : 1.0) * v.TH * v.TW;
        b += 2.0 * 4.0 * (px * v.BN * (pooled ? 1.25 : 1.0) + (bneck ? px : 0.0)) * restored(ex, li, jj);
    }
    return b;
}

double WorkShare::of(const dodt_extractor* ex, const Layer& l) const {
    const size_t li = &l - ex->layers.data();
    if (!per_frame(ex, li)) return steady_frac(ex, l);
    double kept = 0.0, all = 0.0;
    int j = 0;
    for (const Launch* ln : {&l.main, &l.tail}) {
        const int jj = j++;
        if (ln->h_items.empty()) continue;
        const KernelVariant& v = variants()[ln->variant];
        const double units = (double)v.TH * v.TW * v.BN;
        kept += units * items(li, jj);
        all += units * ln->h_items.size();
    }
    return all > 0 ? kept / all : 1.0;
}

}  // namespace dodt

extern "C" {

int dodt_extractor_set_input_support(dodt_extractor* ex, const uint8_t* mask, int rows, int cols,
                                     long long* skipped_items) {
    DODT_REQUIRE(ex, "dodt_extractor_set_input_support: extractor is NULL");
    DODT_REQUIRE(!mask || (rows == ex->H && cols == ex->W),
                 "dodt_extractor_set_input_support: mask is %dx%d, the padded input %dx%d", rows, cols, ex->H, ex->W);
    if (skipped_items) *skipped_items = 0;
    DODT_HIP_CHECK(hipStreamSynchronize(ex->ctx->stream));   // (no launch still reads the old tables)
    free_skip_tables(ex);
    ex->primed = false;
    forget_pairs(ex);
    // fp32 pyramid only (the bf16 / split paths and the plain VGG keep full tables)
    if (!mask || ex->kind != DODT_EXTRACTOR_VGG_PYR || ex->bf16 || ex->first2_variant >= 0) return DODT_OK;
    // each layer's input-dependent outputs, in forward order; a buffer's mask is the OR of its writers so far
    Support bufs[NBUF];
    bufs[X0] = Support(ex->H, ex->W);
    for (int y = 0; y < ex->H; ++y)
        for (int x = 0; x < ex->W; ++x) bufs[X0].at(y, x) = mask[(size_t)y * ex->W + x] != 0;
    long long skipped = 0;
    for (Layer& l : ex->layers) {
        const KernelVariant& lv = variants()[l.main.variant];
        const Support out = l.deconv ? upconv2(bufs[l.src])
                            : lv.family == Family::Wino43 ? wino_blocks(bufs[l.src], 4) : dilate(bufs[l.src], 1);
        Support& d = bufs[l.dst];
        if (d.m.empty()) d = out;
        else
            for (size_t k = 0; k < d.m.size(); ++k) d.m[k] |= out.m[k];
        // the fused (or stand-alone) 2x2 pools behind conv1_2 / conv2_2 / conv3_3
        if (l.pool >= 0) bufs[l.pool] = pool2(out);
        // an item is kept if any output it writes may depend on the input: its conv tile (and with it the pooled
        // outputs of the tile, the NHWC copy and the bottleneck), a transposed conv's 2TH x 2TW outputs
        const SupportSum sum(out);
        double kept_units = 0.0, all_units = 0.0;
        for (Launch* ln : {&l.main, &l.tail}) {
            if (ln->h_items.empty()) continue;
            const KernelVariant& v = variants()[ln->variant];
            const int f = l.deconv ? 2 : 1;
            std::vector<int4> keep;
            for (const int4& it : ln->h_items)
                if (sum.any(f * it.z, f * (it.z + v.TH), f * it.w, f * (it.w + v.TW))) keep.push_back(it);
            const double units = (double)v.TH * v.TW * v.BN;
            kept_units += units * keep.size();
            all_units += units * ln->h_items.size();
            skipped += (long long)(ln->h_items.size() - keep.size());
            ln->n_skip = (int)keep.size();
            if (keep.empty()) continue;
            DODT_HIP_CHECK(hipMalloc(&ln->d_skip, keep.size() * sizeof(int4)));
            DODT_HIP_CHECK(hipMemcpy(ln->d_skip, keep.data(), keep.size() * sizeof(int4), hipMemcpyHostToDevice));
        }
        l.skip_frac = all_units > 0 ? kept_units / all_units : 1.0;
    }
    ex->skip_on = true;
    if (skipped_items) *skipped_items = skipped;
    if (conv_switches().debug_plan)
        for (const Layer& l : ex->layers)
            fprintf(stderr, "[dodt] %-16s skip tables: %d of %d items\n", l.name.c_str(),
                    std::max(l.main.n_skip, 0) + std::max(l.tail.n_skip, 0), l.main.n_items + l.tail.n_items);
    return DODT_OK;
}

int dodt_extractor_set_frame_tables(dodt_extractor* ex, int on, int* enabled) {
    DODT_REQUIRE(ex, "dodt_extractor_set_frame_tables: extractor is NULL");
    if (enabled) *enabled = 0;
    DODT_HIP_CHECK(hipStreamSynchronize(ex->ctx->stream));   // (no launch still reads the old tables)
    free_frame_tables(ex);
    if (!on || !ex->skip_on) return DODT_OK;
    // the layers in the builder's order, none of them block-wise (F(4x4) Winograd); both masks of a frame in LDS
    if ((int)ex->layers.size() != ft::kLayers) return DODT_OK;
    for (const Layer& l : ex->layers)
        for (const Launch* ln : {&l.main, &l.tail})
            if (ln->variant >= 0 && variants()[ln->variant].family == Family::Wino43) return DODT_OK;
    const size_t words = (size_t)ft::level_words(ex->H, ex->W, 0);
    if (words * 8 > 160 * 1024 - 1024) return DODT_OK;
    DODT_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&frame_walk_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)(words * 8)));
    auto alloc = [&](size_t bytes, void** p) {
        hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) e = hipMemset(*p, 0, bytes);
        if (e == hipSuccess) ex->frame_allocs.push_back(*p);
        return e;
    };
    ft::Plan& pl = ex->frame_plan;
    pl.H = ex->H; pl.W = ex->W; pl.frames = ex->batch;
    DODT_HIP_CHECK(alloc((size_t)ex->batch * ft::stash_words(ex->H, ex->W) * 4, (void**)&pl.stash));
    DODT_HIP_CHECK(alloc((size_t)ex->batch * words * 4, (void**)&ex->d_frame_bits));
    DODT_HIP_CHECK(alloc(2 * ft::kTables * sizeof(int), (void**)&ex->d_frame_counts));
    for (size_t li = 0; li < ex->layers.size(); ++li) {
        Layer& l = ex->layers[li];
        int j = 0;
        for (Launch* ln : {&l.main, &l.tail}) {
            ft::Table& t = pl.t[2 * li + j];
            const int jj = j++;
            if (ln->n_skip <= 0) continue;
            const KernelVariant& v = variants()[ln->variant];
            t.items = ln->d_skip;
            t.n = ln->n_skip;
            t.f = l.deconv ? 2 : 1;
            t.th = t.f * v.TH;
            t.tw = t.f * v.TW;
            DODT_HIP_CHECK(alloc(t.n, (void**)&t.now));
            if (li == (size_t)FUSION1) {     // pyramid_fusion1: a set per remembered output pair
                for (int k = 0; k < kOutPairs; ++k) DODT_HIP_CHECK(alloc(t.n, (void**)&ex->out_prev[k][jj]));
            } else {
                DODT_HIP_CHECK(alloc(t.n, (void**)&t.prev));
            }
            DODT_HIP_CHECK(alloc(t.n * sizeof(int4), (void**)&t.run));
            t.count = ex->d_frame_counts + 2 * li + jj;
            DODT_HIP_CHECK(alloc(t.n * sizeof(int4), (void**)&t.restore));
            t.rcount = ex->d_frame_counts + ft::kTables + 2 * li + jj;
            ln->d_run = t.run;
            ln->d_count = t.count;
        }
    }
    DODT_HIP_CHECK(alloc(sizeof(ft::Plan), (void**)&ex->d_frame_plan));
    DODT_HIP_CHECK(hipMemcpy(ex->d_frame_plan, &pl, sizeof(ft::Plan), hipMemcpyHostToDevice));
    // the next forward runs full tables and records its input's items
    ex->primed = false;
    forget_pairs(ex);
    ex->frame_on = true;
    if (enabled) *enabled = 1;
    return DODT_OK;
}

int dodt_extractor_frame_items(dodt_extractor* ex, int* items, int n) {
    DODT_REQUIRE(ex && items && n >= (int)ex->layers.size(),
                 "dodt_extractor_frame_items: items must hold dodt_extractor_layer_count() entries");
    const WorkShare share(ex);
    for (size_t i = 0; i < ex->layers.size(); ++i)
        items[i] = share.per_frame(ex, i) ? share.items(i, 0) + share.items(i, 1) + share.restored(ex, i, 0) +
                                                share.restored(ex, i, 1)
                                          : -1;
    return DODT_OK;
}

int dodt_extractor_frame_split(dodt_extractor* ex, int* computed, int* restored, int n) {
    DODT_REQUIRE(ex && computed && restored && n >= (int)ex->layers.size(),
                 "dodt_extractor_frame_split: computed and restored must hold dodt_extractor_layer_count() entries");
    const WorkShare share(ex);
    for (size_t i = 0; i < ex->layers.size(); ++i) {
        const bool pf = share.per_frame(ex, i);
        computed[i] = pf ? share.items(i, 0) + share.items(i, 1) : -1;
        restored[i] = pf ? share.restored(ex, i, 0) + share.restored(ex, i, 1) : -1;
    }
    return DODT_OK;
}

long long dodt_extractor_store_bytes(const dodt_extractor* ex) { return ex ? (long long)ex->store_bytes : 0; }

}  // extern "C"

namespace {

// the host rule for one layer: restore != nullptr: the two lists; nullptr: run receives their union, in table order
int frame_lists_host(const char* who, const uint8_t* masks, int frames, int rows, int cols, int layer, int th, int tw,
                     const int* items, int n_items, const uint8_t* prev, int* run, int* n_run, int* restore, int* n_restore) {
    DODT_REQUIRE(masks && items && run && n_run && frames >= 1 && n_items >= 0, "%s: NULL argument", who);
    DODT_REQUIRE(rows > 0 && cols > 0 && rows % 8 == 0 && cols % 8 == 0, "%s: masks of %dx%d, not divisible by 8", who, rows,
                 cols);
    DODT_REQUIRE(layer >= 0 && layer < ft::kLayers && th > 0 && tw > 0, "%s: bad layer or tile", who);
    for (int i = 0; i < n_items; ++i)
        DODT_REQUIRE(items[4 * i] >= 0 && items[4 * i] < frames, "%s: item %d names frame %d", who, i, items[4 * i]);
    std::vector<uint8_t> now((size_t)n_items, 0), pv((size_t)n_items, 0);
    if (prev) pv.assign(prev, prev + n_items);
    int count = 0, rcount = 0;
    ft::Plan pl;
    pl.H = rows; pl.W = cols; pl.frames = frames;
    std::vector<uint32_t> stash((size_t)ft::stash_words(rows, cols) * frames);
    pl.stash = stash.data();
    ft::Table& t = pl.t[2 * layer];
    t.items = reinterpret_cast<const int4*>(items);
    t.n = n_items;
    t.f = ft::transposed(layer) ? 2 : 1;
    t.th = t.f * th;
    t.tw = t.f * tw;
    t.now = now.data();
    t.prev = pv.data();
    t.run = reinterpret_cast<int4*>(run);
    t.count = &count;
    t.restore = reinterpret_cast<int4*>(restore);
    t.rcount = &rcount;
    const int words = ft::level_words(rows, cols, 0), p = ft::pitch(cols);
    std::vector<uint32_t> a(words), b(words);
    for (int f = 0; f < frames; ++f) {
        std::fill(a.begin(), a.end(), 0u);
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x)
                if (masks[((size_t)f * rows + y) * cols + x]) a[y * p + (x >> 5)] |= 1u << (x & 31);
        ft::walk(pl, f, a.data(), b.data(), 0, 1, [] {});
    }
    if (!restore) {     // what a forward touches, computed or restored
        for (int i = 0; i < n_items; ++i)
            if (now[i] | pv[i]) memcpy(run + 4 * count++, items + 4 * i, 16);
        *n_run = count;
        return DODT_OK;
    }
    int scan[2];
    if (n_items > 0) ft::compact(t, pv.data(), scan, 0, 1, [] {});
    *n_run = count;
    *n_restore = rcount;
    return DODT_OK;
}

}  // namespace

extern "C" {

int dodt_frame_tables_host(const uint8_t* masks, int frames, int rows, int cols, int layer, int th, int tw,
                           const int* items, int n_items, const uint8_t* prev, int* run, int* n_run) {
    return frame_lists_host("dodt_frame_tables_host", masks, frames, rows, cols, layer, th, tw, items, n_items, prev, run,
                            n_run, nullptr, nullptr);
}

int dodt_frame_restore_host(const int* item, int f, int th, int tw, int bn, int ch0, int rows, int cols, int channels,
                            int pad_top, float* dst, const float* src, float* dst2, const float* src2) {
    DODT_REQUIRE(item && dst && src && (!dst2 == !src2), "dodt_frame_restore_host: NULL argument");
    DODT_REQUIRE(f >= 1 && th > 0 && tw > 0 && tw % 4 == 0 && bn > 0 && bn % 8 == 0 && ch0 % 8 == 0 && rows > 0 && cols > 0 &&
                     cols % 4 == 0 && ch0 + (item[1] + 1) * bn <= channels && item[0] >= 0 && item[2] >= 0 && item[3] >= 0,
                 "dodt_frame_restore_host: bad geometry");
    ft::RestorePlan pl;
    ft::RestoreTable& t = pl.t[0];
    t.H = rows; t.W = cols; t.ch0 = ch0; t.bn = bn; t.f = f; t.th = f * th; t.tw = f * tw;
    if (pad_top < 0) {
        t.dst = dst; t.src = src;
        t.frame_stride = (long long)rows * cols * channels;
        t.pool_dst = dst2; t.pool_src = src2;
        t.pool_frame_stride = (long long)(rows / 2) * (cols / 2) * channels;
    } else {
        DODT_REQUIRE(pad_top < rows, "dodt_frame_restore_host: bad geometry");
        pl.feat = src; pl.bneck = src2;
        pl.pad_top = pad_top; pl.out_h = rows - pad_top; pl.out_c = channels;
    }
    ft::restore_item(pl, t, make_int4(item[0], item[1], item[2], item[3]), dst, dst2, 0, 1);
    return DODT_OK;
}

int dodt_frame_lists_host(const uint8_t* masks, int frames, int rows, int cols, int layer, int th, int tw,
                          const int* items, int n_items, const uint8_t* prev, int* run, int* n_run, int* restore,
                          int* n_restore) {
    DODT_REQUIRE(restore && n_restore, "dodt_frame_lists_host: NULL argument");
    return frame_lists_host("dodt_frame_lists_host", masks, frames, rows, cols, layer, th, tw, items, n_items, prev, run,
                            n_run, restore, n_restore);
}

}  // extern "C"
