// VGG-pyramid feature extractor for gfx950.
//
// Reference topology: avod/core/feature_extractors/bev_vgg_pyramid.py:57-169 and
// img_vgg_pyramid.py:58-171 (see oracle/extractors.py); 1x1 bottleneck
// avod/core/models/dt_rpn_model.py:298-322.  Every conv is slim.conv2d /
// slim.conv2d_transpose with batch-norm (inference form, no gamma, eps 1e-3) and
// ReLU, no bias.
//
// Data layout in HBM: the network input and the returned feature map are NHWC
// float32 (the reference's layout); every activation in between is channel-blocked
// [frame][C/8][H][W][8] ("CB8", see conv_kernels.h), one buffer per pyramid level.
// The decoder's concat inputs are single buffers whose channel planes the two
// producing kernels write directly (conv_k -> planes 0.., upconv_k -> the planes
// after them), so no concat copy exists.  Both frames of a pair are one batch.
//
// This file: the kernel variants and their choice, the small kernels, the extractor's lifecycle, the forward and the
// work accounting.  conv_weights.hip blocks the weights, conv_skip.hip holds the skip tables, the per-frame tables and
// the constants store; extractor.h is the state they share.
#include <cmath>
#include <cstring>

#include <algorithm>
#include <utility>

#include "conv_variants.h"
#include "extractor.h"

using namespace dodt;

const std::vector<KernelVariant>& dodt::variants() {
    static const std::vector<KernelVariant> v = {
        InstSmall<32, 16, 6>::variant(),
        InstSmall<16, 12, 4>::variant(),
        InstSmall<16, 16, 6>::variant(),
        InstSmall<16, 16, 4>::variant(),
        Inst<32, 16, 4, 1, 32, false>::variant(),
        Inst<16, 16, 4, 1, 32, false>::variant(),
        Inst<16, 8, 4, 1, 64, false>::variant(),
        Inst<16, 12, 4, 1, 32, false>::variant(),
        Inst<8, 8, 4, 1, 32, false>::variant(),
        Inst<8, 8, 4, 1, 64, false>::variant(),
        Inst<8, 4, 2, 2, 128, false>::variant(),
        Inst<8, 4, 4, 1, 64, false>::variant(),
        Inst<4, 4, 2, 2, 128, false>::variant(),
        Inst<4, 4, 4, 1, 64, false>::variant(),
        // quarter-size tiles for tail launches (and tiny layers)
        tail_only(Inst<32, 4, 4, 1, 32, false>::variant()),
        tail_only(Inst<16, 4, 4, 1, 32, false>::variant()),
        tail_only(Inst<8, 4, 4, 1, 32, false>::variant()),
        tail_only(Inst<4, 4, 4, 1, 32, false>::variant()),
        Inst<16, 4, 4, 1, 32, true>::variant(),
        Inst<8, 4, 4, 1, 32, true>::variant(),
        Inst<4, 4, 4, 1, 32, true>::variant(),
        Inst<16, 4, 4, 1, 64, true>::variant(),
        Inst<8, 4, 4, 1, 64, true>::variant(),
        Inst<4, 4, 4, 1, 64, true>::variant(),
        InstWino<1, 2>::variant(),    // fp32 Winograd F(2x2,3x3): 16 x 16 px x 32 ch, two workgroups per CU
        InstWino43::variant(),        // F(4x4,3x3): 32 x 16 px x 32 ch, one workgroup per CU
        InstDeconvDma<2>::variant(),  // transposed conv, LDS-DMA staged: 16 x 16 input px x 32 ch
        InstDeconvDma<1>::variant(),  //   ... x 16 ch: twice the items, for layers with few of them
    };
    static const std::vector<KernelVariant> all = [] {
        std::vector<KernelVariant> a = v;
        for (const KernelVariant& b : dodt::bf16_variants()) a.push_back(b);
        for (const KernelVariant& b : dodt::split_variants()) a.push_back(b);
        return a;
    }();
    return all;
}

// which form the fp32 3x3 stride-1 layers take in this process (read once)
extern "C" int dodt_conv_mode(void) {
    static const int mode = [] {
        const char* e = getenv("DODT_CONV_WINO");
        const int m = e ? atoi(e) : DODT_CONV_MODE_DEFAULT;
        return (m == 0 || m == 2 || m == 4) ? m : DODT_CONV_MODE_DEFAULT;
    }();
    return mode;
}

// every switch the conv path reads, once per process; unset or anything but 0 leaves a form on
const ConvSwitches& dodt::conv_switches() {
    static const ConvSwitches s = [] {
        auto on = [](const char* name) {
            const char* e = getenv(name);
            return !(e && atoi(e) == 0);
        };
        ConvSwitches c;
        c.wino = dodt_conv_mode();
        c.deconv_dma = on("DODT_CONV_DECONV_DMA");
        c.bf16_dma = on("DODT_CONV_BF16_DMA");
        c.bf16_stream = on("DODT_CONV_BF16_STREAM");
        c.bf16_first2 = on("DODT_CONV_BF16_FIRST2");
        c.bf16_xcd = on("DODT_CONV_BF16_XCD");
        c.f32_xcd = on("DODT_CONV_F32_XCD");
        const char* dbg = getenv("DODT_CONV_DEBUG");
        c.debug = dbg ? atoi(dbg) : 0;
        c.stamp_layer = getenv("DODT_CONV_STAMP_LAYER");
        c.debug_plan = getenv("DODT_DEBUG_PLAN") != nullptr;
        return c;
    }();
    return s;
}

namespace {

// One work queue per group of blocks that share an XCD (conv_bf16_dma.h) in the persistent LDS-DMA kernels.  fp32:
// both stacks 2.90 -> 2.80 ms alone, nothing in the pipeline, half the excess fabric traffic.
bool variant_xcd_queue(const KernelVariant& v) {
    switch (v.family) {
        case Family::Bf16Dma:
        case Family::Bf16Stream:
        case Family::Bf16First2: return conv_switches().bf16_xcd;
        case Family::DeconvDma: return v.bf16 ? conv_switches().bf16_xcd : conv_switches().f32_xcd;
        case Family::Wino22: return conv_switches().f32_xcd;
        case Family::Wino43:
        case Family::Direct:
        case Family::SmallCin: return false;
    }
    return false;
}

// ---------------------------------------------------------------------------
// Which kernel a layer runs: pick_variant asks the families' rules in order; each returns a table index or -1.
// The measurements behind the rules: DESIGN.md section 5.
// ---------------------------------------------------------------------------
struct LayerShape {
    bool deconv;
    int H, W, Cin, Cout;
    bool bf16;   // bf16 activations: the bf16 and the split extractor
    int parts;
    int batch, num_cus;
};

long variant_items(const KernelVariant& v, const LayerShape& s) {
    return (long)dodt::ceil_div(s.H, v.TH) * dodt::ceil_div(s.W, v.TW) * (s.Cout / v.BN) * s.batch;
}

// fp32 3x3 stride-1 convs with >= 4 chunks of input channels run as Winograd.  mode 2 (default):
// F(2x2,3x3), two workgroups per CU -- both stacks 3.0 ms against the direct kernels' 4.8, rounding noise at their
// level.  mode 4: F(4x4,3x3) -- 2.8 ms, but its fp32 accumulation in the transformed domain is 7x noisier, which
// costs a third of the end-to-end agreement with the exact result: opt-in.  mode 0: the direct kernels.
int pick_wino(const LayerShape& s, int mode) {
    if (mode == 0 || s.deconv || s.bf16 || s.parts != 1 || s.Cin < 32 || s.Cin % 16 != 0) return -1;
    const auto& vs = variants();
    int best = -1;
    for (size_t i = 0; i < vs.size(); ++i) {
        if (s.Cout % vs[i].BN != 0) continue;
        if (vs[i].family == Family::Wino43 && mode == 4) return (int)i;
        if (vs[i].family == Family::Wino22 && (best < 0 || vs[i].BN > vs[best].BN)) best = (int)i;
    }
    return best;
}

// Transposed convs, fp32 and bf16: the LDS-DMA staged kernel (deconv_kernel.h).  32-channel tiles unless that leaves
// fewer than four items per CU (the CUs are MFMA-bound: what counts is how evenly the items spread).
int pick_deconv_dma(const LayerShape& s) {
    if (!s.deconv || s.parts != 1 || s.Cin < 32 || s.Cin % 16 != 0) return -1;
    const auto& vs = variants();
    const int n32 = dodt::ceil_div(s.H, 16) * dodt::ceil_div(s.W, 16) * (s.Cout / 32) * s.batch;
    const int want_bn = (s.Cout % 32 == 0 && n32 >= 4 * s.num_cus) ? 32 : 16;
    for (size_t i = 0; i < vs.size(); ++i)
        if (vs[i].family == Family::DeconvDma && vs[i].bf16 == s.bf16 && vs[i].BN == want_bn && s.Cout % want_bn == 0)
            return (int)i;
    return -1;
}

// bf16 3x3 stride-1 convs: the LDS-DMA staged kernels (conv_bf16_dma.h: scalar-only copy issue between the MFMAs,
// accumulators pinned in place; stacks alone as fast as the template's bf16 instantiation, frame-pair pipeline 7 %
// faster).
//  * The level-1 layers (32 output channels, 2 / 4 chunks): the streaming kernel.
//  * 8-row tiles (three workgroups per CU) only where the 16-row tiles give fewer than 1.6 items per CU -- the
//    88 x 100 / 45 x 150 maps of the deepest level: conv4_2 34 -> 30 us; at 1.9 items per CU (the image net's level
//    3) they are slower, 26 -> 29 us.
//  * Among the tiles of that height the widest channel tile that still leaves four items per CU (two resident
//    workgroups, two rounds); if none does, the one with the most items.
int pick_bf16_dma(const LayerShape& s, bool stream) {
    if (!s.bf16 || s.parts != 1 || s.deconv || s.Cin < 32 || s.Cin % 32 != 0) return -1;
    const auto& vs = variants();
    if (stream && s.Cout == 32)
        for (size_t i = 0; i < vs.size(); ++i)
            if (vs[i].family == Family::Bf16Stream && vs[i].stream_nch * 16 == s.Cin) return (int)i;
    long n16 = 0, n8 = 0;
    for (const KernelVariant& v : vs)
        if (v.family == Family::Bf16Dma && s.Cout % v.BN == 0) {
            if (v.TH == 16) n16 = std::max(n16, variant_items(v, s));
            if (v.TH == 8) n8 = std::max(n8, variant_items(v, s));
        }
    const bool rows8 = n8 > 0 && n16 < 8L * s.num_cus / 5;
    const long enough_items = 4L * s.num_cus;
    int best = -1;
    long best_n = 0;
    for (size_t i = 0; i < vs.size(); ++i) {
        if (vs[i].family != Family::Bf16Dma || s.Cout % vs[i].BN != 0 || (vs[i].TH == 8) != rows8) continue;
        const long n = variant_items(vs[i], s);
        const bool enough = n >= enough_items, best_enough = best_n >= enough_items;
        if (best < 0 || (enough && !best_enough) || (enough && best_enough && vs[i].BN > vs[best].BN) ||
            (!enough && !best_enough && n > best_n)) {
            best = (int)i; best_n = n;
        }
    }
    return best;
}

// The register-staged template and the first-layer kernel: the cheapest tiling by a cost model.  Which model is
// measured.  fp32 and the first layer: padded pixels, with a mild preference for more work per staged byte (the
// round model's choices run a lone net 9 % faster but the frame-pair pipeline 4 % slower).  bf16 and split: the
// round model (stacks 15 % faster alone, pipeline 4-6 % faster) -- workgroups sharing a CU share its matrix pipe,
// so a layer takes ceil(items / CUs) item times; an item = its 32x32 MFMA tiles over the variant's in-tile
// efficiency (2x2 tiles per wave 1.0, 2 tiles 0.9, 1 tile 0.8).  Ties go to the entry that stands first.
int pick_direct(const LayerShape& s) {
    const auto& vs = variants();
    const bool small = s.Cin < dodt::kCK;
    int best = -1;
    double best_cost = 1e300;
    for (size_t i = 0; i < vs.size(); ++i) {
        const KernelVariant& v = vs[i];
        if (v.family != (small ? Family::SmallCin : Family::Direct)) continue;
        if (v.deconv != s.deconv || v.tail_only || v.bf16 != s.bf16 || v.parts != s.parts || s.Cout % v.BN != 0) continue;
        // the chunk pipeline needs >= 2 chunks (8 channels fp32, 16 channels bf16) per item
        if (small ? (s.Cin != v.CK || s.Cout != 32) : (s.Cin % v.CK != 0 || s.Cin < 32)) continue;
        double cost;
        if (!s.bf16 || small) {
            const double padded = (double)dodt::ceil_div(s.H, v.TH) * v.TH * dodt::ceil_div(s.W, v.TW) * v.TW;
            cost = padded * (1.0 + 0.04 / v.MTB + 1.0 / v.BN);
        } else {
            const double items = (double)dodt::ceil_div(s.H, v.TH) * dodt::ceil_div(s.W, v.TW) * s.batch * (s.Cout / v.BN);
            const int wave_tiles = s.deconv ? 4 * (v.BN / 32 / v.WN) : (v.MTB / v.WM) * (v.BN / 32 / v.WN);
            const double eff = wave_tiles >= 4 ? 1.0 : wave_tiles >= 2 ? 0.9 : 0.8;
            const double units = (double)(v.TW * v.TH / 32) * (v.BN / 32);
            cost = std::ceil(items / s.num_cus) * units / eff;
        }
        if (cost < best_cost) { best_cost = cost; best = (int)i; }
    }
    return best;
}

int pick_variant(const LayerShape& s) {
    const ConvSwitches& sw = conv_switches();
    int i = pick_wino(s, sw.wino);
    if (i < 0 && sw.deconv_dma) i = pick_deconv_dma(s);
    if (i < 0 && sw.bf16_dma) i = pick_bf16_dma(s, sw.bf16_stream);
    return i >= 0 ? i : pick_direct(s);
}

// ---------------------------------------------------------------------------
// small HBM-bound helpers
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
maxpool2x2_kernel(const float* __restrict__ in, int H, int W, int planes,
                  long long in_frame_stride, float* __restrict__ out, int frames) {
    // CB8 in / CB8 out; one lane per (plane, output pixel, half of the 8 channels);
    // VALID 2x2 stride 2.  Reads the first `planes` planes of the (wider) input.
    const int OH = H / 2, OW = W / 2;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)frames * planes * OH * OW * 2;
    if (t >= total) return;
    const int g = (int)(t & 1);
    long long r = t >> 1;
    const int ox = (int)(r % OW); r /= OW;
    const int oy = (int)(r % OH); r /= OH;
    const int pl = (int)(r % planes);
    const int f = (int)(r / planes);
    const float* p = in + (size_t)f * in_frame_stride + (size_t)pl * H * W * 8 +
                     ((size_t)(2 * oy) * W + 2 * ox) * 8 + g * 4;
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 8);
    const float4 c = *reinterpret_cast<const float4*>(p + (size_t)W * 8);
    const float4 d = *reinterpret_cast<const float4*>(p + (size_t)W * 8 + 8);
    float4 o;
    o.x = fmaxf(fmaxf(a.x, b.x), fmaxf(c.x, d.x));
    o.y = fmaxf(fmaxf(a.y, b.y), fmaxf(c.y, d.y));
    o.z = fmaxf(fmaxf(a.z, b.z), fmaxf(c.z, d.z));
    o.w = fmaxf(fmaxf(a.w, b.w), fmaxf(c.w, d.w));
    reinterpret_cast<float4*>(out)[t] = o;   // out index == t by construction
}

// 1x1 conv to one channel + batch-norm + ReLU; 8 lanes per pixel, float4 each
__global__ void __launch_bounds__(256)
bottleneck32_kernel(const float* __restrict__ in, long long n_pix, const float* __restrict__ w,
                    float scale, float shift, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long pix = t >> 3;
    const int g = (int)(t & 7);
    float s = 0.0f;
    if (pix < n_pix) {
        const float4 v = reinterpret_cast<const float4*>(in)[pix * 8 + g];
        const float4 k = reinterpret_cast<const float4*>(w)[g];
        s = ((v.x * k.x + v.y * k.y) + v.z * k.z) + v.w * k.w;
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    if (pix < n_pix && g == 0) out[pix] = fmaxf(s * scale + shift, 0.0f);
}

__global__ void __launch_bounds__(256)
copy_rows_kernel(const float4* __restrict__ src, float4* __restrict__ dst, long long n4_per_frame,
                 long long src_frame_stride4, long long dst_frame_stride4, int frames) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n4_per_frame * frames) return;
    const int f = (int)(t / n4_per_frame);
    const long long i = t - (long long)f * n4_per_frame;
    dst[f * dst_frame_stride4 + i] = src[f * src_frame_stride4 + i];
}

// tf.image.resize_bilinear (TF 1.3 legacy sampling, align_corners = False: src = dst * in/out)
// of the CB8 conv4_3 map to the NHWC feature map the plain-VGG extractors return
// (bev_vgg.py:102-112, img_vgg.py:104-114), with the 1x1 bottleneck (rpn_model.py:251-267)
// on the upsampled pixel fused in.  C / 4 lanes per output pixel, one float4 of channels each:
// a wave stores 1 KB of contiguous NHWC output per instruction; the source map (9-12 MB)
// stays in L2.  HBM-bound on the output write.  float32, unfused, TF's operation order.
template <int LPP>   // lanes per pixel = C / 4
__global__ void __launch_bounds__(256)
upsample_bilinear_cb8_kernel(const float* __restrict__ in, int IH, int IW, long long in_frame_stride,
                             int OH, int OW, int frames, float* __restrict__ out,
                             const float* __restrict__ bneck_w, float bneck_scale,
                             float bneck_shift, float* __restrict__ bneck_out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long pix = t / LPP;
    const int l = (int)(t % LPP);
    const long long n_pix = (long long)frames * OH * OW;
    const bool ok = pix < n_pix;
    float dot = 0.0f;
    if (ok) {
        const int f = (int)(pix / ((long long)OH * OW));
        const int r = (int)(pix - (long long)f * OH * OW);
        const int oy = r / OW, ox = r - oy * OW;
        const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;
        const float fy = (float)oy * sy, fx = (float)ox * sx;
        const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
        const int y1 = min(y0 + 1, IH - 1), x1 = min(x0 + 1, IW - 1);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const float* base = in + (size_t)f * in_frame_stride + (size_t)(l >> 1) * IH * IW * 8 +
                            (l & 1) * 4;
        const f32x4 tl = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * IW + x0) * 8);
        const f32x4 tr = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * IW + x1) * 8);
        const f32x4 bl = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * IW + x0) * 8);
        const f32x4 br = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * IW + x1) * 8);
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float top = tl[k] + (tr[k] - tl[k]) * lx;
            const float bot = bl[k] + (br[k] - bl[k]) * lx;
            v[k] = top + (bot - top) * ly;
        }
        *reinterpret_cast<f32x4*>(out + (size_t)pix * (LPP * 4) + l * 4) = v;
        if (bneck_out) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(bneck_w + l * 4);
            dot = ((v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]) + v[3] * w[3];
        }
    }
    if (bneck_out) {
#pragma unroll
        for (int m = 1; m < LPP; m <<= 1) dot += __shfl_xor(dot, m, 64);
        if (ok && l == 0) bneck_out[pix] = fmaxf(dot * bneck_scale + bneck_shift, 0.0f);
    }
}

int find_layer(dodt_extractor* ex, const char* name) {
    for (size_t i = 0; i < ex->layers.size(); ++i)
        if (ex->layers[i].name == name) return (int)i;
    return -1;
}

// DODT_CONV_DEBUG / DODT_CONV_STAMP_LAYER: read back what the launch just left in the diagnostic words (waits for it)
void report_launch(const dodt_extractor* ex, const Layer& l, const KernelVariant& v, const ConvArgs& a, int grid_x) {
    if (a.debug & 32) {
        int h[74];
        (void)hipStreamSynchronize(ex->ctx->stream);
        (void)hipMemcpy(h, ex->d_counters + 64 + 32, sizeof(h), hipMemcpyDeviceToHost);
        fprintf(stderr, "[dodt] %s step stamps (cycles): copies | transform | MFMAs | wait copies | barrier | step\n",
                l.name.c_str());
        for (int k = 0; k < 12; ++k)
            fprintf(stderr, "[dodt]   step %2d: %6d %6d %6d %6d %6d   next-top %6d\n", k, h[k * 6 + 1] - h[k * 6],
                    h[k * 6 + 2] - h[k * 6 + 1], h[k * 6 + 3] - h[k * 6 + 2], h[k * 6 + 4] - h[k * 6 + 3],
                    h[k * 6 + 5] - h[k * 6 + 4], k < 11 ? h[(k + 1) * 6] - h[k * 6] : 0);
        if (h[73] != h[72])
            fprintf(stderr, "[dodt]   steps 0..11: %d stamp ticks in %d ticks of the 100 MHz clock (%.0f MHz)\n",
                    h[66] - h[0], h[73] - h[72], 100.0 * (h[66] - h[0]) / (h[73] - h[72]));
    }
    const bool bf16_dma = v.family == Family::Bf16Dma || v.family == Family::Bf16Stream || v.family == Family::Bf16First2;
    if ((a.debug & 128) && bf16_dma) {   // diagnostic: when the workgroups of this launch started and ended
        std::vector<int> h(4 * grid_x);
        (void)hipStreamSynchronize(ex->ctx->stream);
        (void)hipMemcpy(h.data(), ex->d_counters + 64 + 256, h.size() * sizeof(int), hipMemcpyDeviceToHost);
        int t0 = h[0], s_max = h[0], f_max = h[1], e_min = h[2], e_max = h[2], items[8] = {};
        double first_sum = 0, run_sum = 0;
        for (int b = 0; b < (int)grid_x; ++b) {
            t0 = std::min(t0, h[4 * b]); s_max = std::max(s_max, h[4 * b]);
            f_max = std::max(f_max, h[4 * b + 1]);
            e_min = std::min(e_min, h[4 * b + 2]); e_max = std::max(e_max, h[4 * b + 2]);
            items[std::min(h[4 * b + 3], 7)]++;
            first_sum += (h[4 * b + 1] - h[4 * b]) / 100.0;
            run_sum += (h[4 * b + 2] - h[4 * b + 1]) / 100.0 / std::max(h[4 * b + 3], 1);
        }
        fprintf(stderr, "[dodt] %-16s %4d wgs, %5d items x %d chunks: last start +%.2f us, last first-step +%.2f, first end +%.2f, "
                "last end +%.2f; mean start->first step %.2f us, mean per item %.2f us; wgs by item count:",
                l.name.c_str(), (int)grid_x, a.n_items, a.Cin / 16, (s_max - t0) / 100.0, (f_max - t0) / 100.0,
                (e_min - t0) / 100.0, (e_max - t0) / 100.0, first_sum / grid_x, run_sum / grid_x);
        for (int k = 0; k < 8; ++k) if (items[k]) fprintf(stderr, " %d:%d", k, items[k]);
        int mt[2] = {0, 0};
        (void)hipMemcpy(mt, ex->d_counters + 64 + 250, sizeof(mt), hipMemcpyDeviceToHost);
        fprintf(stderr, "; shader clock of workgroup 1: %.2f GHz\n", (mt[1] - mt[0]) / ((h[4 + 2] - h[4 + 0]) * 10.0));
    }
    if (a.debug & 8) {   // diagnostic: print the in-kernel clock of this launch
        unsigned long long h[2] = {0, 0};
        (void)hipStreamSynchronize(ex->ctx->stream);
        (void)hipMemcpy(h, ex->d_counters + 96, sizeof(h), hipMemcpyDeviceToHost);
        if (h[1])
            fprintf(stderr, "[dodt] %-16s wg0: %.1f us, shader clock %.3f GHz\n", l.name.c_str(),
                    h[1] / 100.0, (double)h[0] / h[1] * 0.1);
    }
}

// persistent workgroups: as many as stay resident on num_cus CUs, each walks items with that stride
int launch_grid(const KernelVariant& v, int n_items, int num_cus) {
    // (the first-layer kernel is persistent since round 4: three workgroups per CU by its registers)
    const int bpc = v.family == Family::SmallCin ? 3 : v.blocks_per_cu;
    return std::min(n_items, num_cus * bpc);
}

// which: 0 the layer's main launch, 1 its tail
int run_launch(const dodt_extractor* ex, const Pass& p, const Layer& l, int which,
               float* override_out, int out_y0, int out_h, float* bneck_out, int pool_dst, const Layer* folded = nullptr) {
    // folded: conv1_1, computed inside this launch of conv1_2 (same items and weights as conv1_2's streaming kernel)
    const Launch& ln = which ? l.tail : l.main;
    const size_t li = &l - ex->layers.data();
    const ItemTable& t = p.table[li][which];
    const KernelVariant& v = variants()[folded ? ex->first2_variant : ln.variant];
    const int src_id = folded ? folded->src : l.src;
    const Buffer& src = ex->buf[src_id];
    const Buffer& dst = ex->buf[l.dst];
    ConvArgs a;
    a.in = p.map[src_id];
    a.out = override_out ? override_out : p.map[l.dst];
    a.w = ln.d_w ? ln.d_w : l.main.d_w;
    a.scale = l.d_scale;
    a.shift = l.d_shift;
    a.H = l.H;
    a.W = l.W;
    a.Cin = l.Cin;
    a.Cout = l.Cout;
    a.in_ld = src.C;
    a.in_coff = folded ? folded->src_coff : l.src_coff;
    a.out_ld = dst.C;
    a.out_coff = l.dst_coff;
    a.in_frame_stride = (long long)src.frame_floats();
    a.out_frame_stride = override_out ? (long long)out_h * dst.W * dst.C : (long long)dst.frame_floats();
    a.tiles_x = dodt::ceil_div(l.W, v.TW);
    a.tiles_y = dodt::ceil_div(l.H, v.TH);
    a.relu = 1;
    a.out_y0 = out_y0;
    a.out_nhwc = override_out ? 1 : 0;
    a.debug = conv_switches().debug;
    // in-kernel step stamps of one layer's launch (+ DODT_CONV_DEBUG=64: the streaming kernel's producer wave)
    if (conv_switches().stamp_layer && l.name == conv_switches().stamp_layer) a.debug |= 32;
    a.counter = ex->d_counters + 2 * li + which;
    a.counter_base = ex->d_counters + 64;
    // (eight counters, 64 bytes apart, per layer: words 2048.. of the block)
    a.xcd_counters = variant_xcd_queue(v) ? ex->d_counters + 2048 + 128 * li : nullptr;
    // the first-layer kernel derives a full table's coordinates from the item index (no table load ahead of its patch)
    a.items = v.family == Family::SmallCin && t.dense && t.n == a.tiles_x * a.tiles_y * p.frames ? nullptr : t.items;
    a.n_items = t.n;
    if (a.n_items == 0) return DODT_OK;   // every item of the launch skipped
    // per-frame tables: the builder's launches ahead in the stream wrote this forward's items and their count
    a.n_items_dev = t.n_dev;
    a.in_part_stride = (long long)src.frame_floats() * p.frames;
    a.out_part_stride = (long long)dst.frame_floats() * p.frames;
    a.pool_part_stride = pool_dst >= 0 ? (long long)ex->buf[pool_dst].frame_floats() * p.frames : 0;
    a.pool_out = pool_dst >= 0 ? p.map[pool_dst] : nullptr;
    a.pool_frame_stride = pool_dst >= 0 ? (long long)ex->buf[pool_dst].frame_floats() : 0;
    a.bneck_w = bneck_out ? ex->d_bneck_w : nullptr;
    a.bneck_out = bneck_out;
    a.bneck_scale = ex->bneck_scale;
    a.bneck_shift = ex->bneck_shift;
    a.bneck_frame_stride = (long long)out_h * dst.W;
    a.zeros = ex->d_zeros;
    a.first_w = folded ? folded->d_first_w : nullptr;
    a.first_scale = folded ? folded->d_scale : nullptr;
    a.first_shift = folded ? folded->d_shift : nullptr;
    const int grid_x = launch_grid(v, a.n_items, ex->num_cus);
    dim3 grid(grid_x, 1);
    v.launch(a, grid, ex->ctx->stream);
    DODT_LAUNCH_CHECK();
    if (a.debug & (32 | 128 | 8)) report_launch(ex, l, v, a, grid_x);
    return DODT_OK;
}

// a variant's waves hold both rows of every 2x2 pooling window (conv_kernels.h kCanPool)
bool variant_can_pool(const KernelVariant& v) {
    switch (v.family) {
        case Family::Wino22:
        case Family::Wino43: return true;   // a lane's output block is whole 2x2 pooling windows
        case Family::SmallCin:
        case Family::DeconvDma: return false;
        case Family::Direct:
        case Family::Bf16Dma:
        case Family::Bf16Stream:
        case Family::Bf16First2: break;
    }
    const int rows_per_mt = 32 / v.TW, mt = v.MTB / v.WM;
    return !v.deconv && (rows_per_mt >= 2 || mt % 2 == 0) && v.TH % 2 == 0;
}

bool layer_can_pool(const Layer& l) {
    return variant_can_pool(variants()[l.main.variant]) &&
           (l.tail.n_items == 0 || variant_can_pool(variants()[l.tail.variant]));
}

// pool_dst >= 0: the layer also writes its 2x2 max pool into that buffer
int run_layer(const dodt_extractor* ex, const Pass& p, const Layer& l, float* override_out, int out_y0, int out_h,
              float* bneck_out = nullptr, int pool_dst = -1, const Layer* folded = nullptr) {
    if (p.timed && folded) {      // (the folded layer has no time of its own)
        DODT_HIP_CHECK(hipEventRecord(folded->ev0, ex->ctx->stream));
        DODT_HIP_CHECK(hipEventRecord(folded->ev1, ex->ctx->stream));
    }
    if (p.timed) DODT_HIP_CHECK(hipEventRecord(l.ev0, ex->ctx->stream));
    int rc = run_launch(ex, p, l, 0, override_out, out_y0, out_h, bneck_out, pool_dst, folded);
    if (rc == DODT_OK && l.tail.variant >= 0)
        rc = run_launch(ex, p, l, 1, override_out, out_y0, out_h, bneck_out, pool_dst);
    if (rc == DODT_OK && p.timed) DODT_HIP_CHECK(hipEventRecord(l.ev1, ex->ctx->stream));
    return rc;
}

// the __global__ function a variant launches (what rocprofv3 --kernel-trace lists)
const char* kernel_name(const KernelVariant& v) {
    switch (v.family) {
        case Family::Direct: return "conv3x3_mfma_kernel";
        case Family::SmallCin: return "conv3x3_small_cin_kernel";
        case Family::Wino22: return "wino3x3_f32_kernel";
        case Family::Wino43: return "wino43_f32_kernel";
        case Family::DeconvDma: return "deconv3x3_dma_kernel";
        case Family::Bf16Dma: return "conv3x3_bf16_dma_kernel";
        case Family::Bf16Stream: return "conv3x3_bf16_stream_kernel";
        case Family::Bf16First2: return "conv3x3_bf16_first2_kernel";
    }
    return "";
}

// frac: share of the layer's work items that run (skip tables: Layer::skip_frac)
double layer_direct_flops(const dodt_extractor* ex, const Layer& l, double frac = 1.0) {
    return 2.0 * l.H * l.W * (double)l.Cout * 9.0 * l.real_cin * ex->batch * frac;
}

// FLOPs the matrix pipe executes for a layer: the Winograd kernels multiply 36 times per 4x4
// outputs and channel pair (F(4x4,3x3)) or 16 times per 2x2 (F(2x2,3x3)) where the direct form
// needs 144 / 36; split mode issues three bf16 MFMAs per product term
double layer_executed_flops(const dodt_extractor* ex, const Layer& l, double frac = 1.0) {
    const KernelVariant& kv = variants()[l.main.variant];
    const double direct = layer_direct_flops(ex, l, frac);
    switch (kv.family) {
        case Family::Wino22: return direct * (16.0 / 36.0);
        case Family::Wino43: return direct * (36.0 / 144.0);
        default: return kv.parts == 2 ? 3.0 * direct : direct;
    }
}

// algorithmic HBM bytes of a layer: input map and weights read once, output map (and its pooled
// copy) written once; split mode keeps two bf16 maps (hi + lo) and two bf16 weight sets per tensor;
// frac < 1 (skip tables): that share of the maps
double layer_bytes(const dodt_extractor* ex, const Layer& l, double frac = 1.0) {
    const Buffer& src = ex->buf[l.src];
    const Buffer& dst = ex->buf[l.dst];
    const double in_e = src.bf16 ? 2.0 * src.parts : 4.0;
    const double out_e = dst.bf16 ? 2.0 * dst.parts : 4.0;
    const double w_e = (ex->bf16 && &l != &ex->layers[CONV1_1]) ? 2.0 * ex->parts : 4.0;
    const double oh = l.deconv ? 2.0 * l.H : l.H, ow = l.deconv ? 2.0 * l.W : l.W;
    double b = ex->batch * ((double)l.H * l.W * l.real_cin * in_e + oh * ow * l.Cout * out_e) +
               9.0 * l.real_cin * l.Cout * w_e;
    // conv1_1 folded into conv1_2's launch: conv1_1's map is neither written nor read
    if (ex->first2_variant >= 0 && &l == &ex->layers[CONV1_1]) b -= ex->batch * oh * ow * l.Cout * out_e;
    if (ex->first2_variant >= 0 && &l == &ex->layers[CONV1_2]) b -= ex->batch * (double)l.H * l.W * l.real_cin * in_e;
    if (l.pool >= 0)
        b += ex->batch * std::floor(oh / 2) * std::floor(ow / 2) * l.Cout * out_e;
    const double w_bytes = 9.0 * l.real_cin * l.Cout * w_e;
    return (b - w_bytes) * frac + w_bytes;
}

// Work items of a layer.  The main launch walks big tiles; when their count leaves the
// last round of the persistent grid mostly idle, the surplus tiles are handed to a tail
// launch that cuts each of them into smaller tiles (same TW; fewer rows and/or channels),
// so the tail costs a fraction of a round.  Every output element is still summed by one
// workgroup in one fixed order: results do not depend on how a layer is cut.
void plan_layer(Layer& l, int batch, int num_cus, bool allow_tail, std::vector<int4>& main_items,
                std::vector<int4>& tail_items) {
    const auto& vs = variants();
    const KernelVariant& v = vs[l.variant];
    const int tx = dodt::ceil_div(l.W, v.TW), ty = dodt::ceil_div(l.H, v.TH), nt = l.Cout / v.BN;
    main_items.clear();
    tail_items.clear();
    if (variant_xcd_queue(v)) {
        // XCD-grouped queue (conv_bf16_dma.h): the channel tiles of a pixel tile next to each other
        for (int f = 0; f < batch; ++f)
            for (int y = 0; y < ty; ++y)
                for (int x = 0; x < tx; ++x)
                    for (int n = 0; n < nt; ++n) main_items.push_back(make_int4(f, n, y * v.TH, x * v.TW));
    } else {
        for (int f = 0; f < batch; ++f)
            for (int n = 0; n < nt; ++n)
                for (int y = 0; y < ty; ++y)
                    for (int x = 0; x < tx; ++x) main_items.push_back(make_int4(f, n, y * v.TH, x * v.TW));
    }
    l.main.variant = l.variant;
    l.tail.variant = -1;
    if (v.family != Family::Direct) return;   // (only the template has quarter-size companions)
    const int n = (int)main_items.size();
    const int G = num_cus * v.blocks_per_cu;
    const int surplus = n % G;
    if (!allow_tail || n < G || surplus == 0) return;
    // companion: a template entry of the same kind and data type, same TW, dividing the big tile, as small as possible
    int best = -1, best_units = 1 << 30;
    const int big_units = (v.TW * v.TH / 32) * (v.BN / 32);
    for (size_t i = 0; i < vs.size(); ++i) {
        const KernelVariant& c = vs[i];
        if (c.family != Family::Direct || c.deconv != v.deconv || c.bf16 != v.bf16 || c.parts != v.parts) continue;
        if (c.TW != v.TW || v.TH % c.TH != 0 || v.BN % c.BN != 0) continue;
        const int units = (c.TW * c.TH / 32) * (c.BN / 32);
        if (units < big_units && units < best_units) { best = (int)i; best_units = units; }
    }
    if (best < 0) return;
    const KernelVariant& c = vs[best];
    const int ry = v.TH / c.TH, rn = v.BN / c.BN;
    std::vector<int4> small;
    for (int k = n - surplus; k < n; ++k) {
        const int4 b = main_items[k];
        for (int jn = 0; jn < rn; ++jn)
            for (int jy = 0; jy < ry; ++jy)
                if (b.z + jy * c.TH < l.H)
                    small.push_back(make_int4(b.x, b.y * rn + jn, b.z + jy * c.TH, b.w));
    }
    // cost of the tail in rounds of the main launch (one round = blocks_per_cu big tiles per
    // CU).  Measured: small tiles sharing a CU run at the big tiles' rate, a lone small tile
    // per CU at ~0.78 of it.
    const double share = (double)best_units / (v.blocks_per_cu * big_units);
    double cost_small;
    if ((int)small.size() <= num_cus)
        cost_small = share / 0.78;
    else
        cost_small = dodt::ceil_div((int)small.size(), num_cus * c.blocks_per_cu) *
                     c.blocks_per_cu * share;
    cost_small += 0.04;   // second launch
    if (cost_small >= 1.0) return;
    main_items.resize(n - surplus);
    tail_items = small;
    l.tail.variant = best;
}

int run_pool(const dodt_extractor* ex, const Pass& p, int src, int dst) {
    const Buffer& s = ex->buf[src];
    const Buffer& d = ex->buf[dst];
    const int planes = d.C / 8;
    const long long total = (long long)p.frames * planes * d.H * d.W * 2;
    hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       ex->ctx->stream, p.map[src], s.H, s.W, planes, (long long)s.frame_floats(),
                       p.map[dst], p.frames);
    DODT_LAUNCH_CHECK();
    return DODT_OK;
}

// one forward: d_x0 (or the X0 buffer where it is NULL) through the tables choose_tables picks
int forward(dodt_extractor* ex, const float* d_in, const float* d_x0, float* d_feat_out, float* d_bottleneck_out,
            bool timed);

}  // namespace

int dodt::fused_pool_buffer(const Layer& l) {
    return layer_can_pool(l) ? l.pool : -1;
}

bool dodt::bneck_fused(const Layer& last) {
    return variants()[last.main.variant].BN == 32 && (last.tail.n_items == 0 || variants()[last.tail.variant].BN == 32);
}

int dodt::run_layers(const dodt_extractor* ex, const Pass& p, float* d_feat_out, float* d_bottleneck_out) {
    hipStream_t s = ex->ctx->stream;
    int rc;
    const std::vector<Layer>& ls = ex->layers;
    if (ex->bf16)   // there is no stand-alone pool kernel for bf16 maps
        for (int id : {CONV1_2, CONV2_2, CONV3_3})
            DODT_REQUIRE(fused_pool_buffer(ls[id]) >= 0, "bf16 extractor: layer %s cannot pool in its epilogue",
                         ls[id].name.c_str());
    for (int id = ex->first2_variant >= 0 ? CONV1_2 : CONV1_1; id <= CONV4_3; ++id) {
        const Layer& l = ls[id];
        // conv1_1 folded into conv1_2's launch; a conv that a 2x2 max pool follows pools in its epilogue when its
        // tiling allows
        const Layer* folded = id == CONV1_2 && ex->first2_variant >= 0 ? &ls[CONV1_1] : nullptr;
        const int pool_dst = folded ? l.pool : fused_pool_buffer(l);
        if ((rc = run_layer(ex, p, l, nullptr, 0, 0, nullptr, pool_dst, folded))) return rc;
        if (l.pool >= 0 && pool_dst < 0 && (rc = run_pool(ex, p, l.dst, l.pool))) return rc;
    }
    if (ex->kind == DODT_EXTRACTOR_VGG) {
        // bev_vgg.py:102-112 / img_vgg.py:104-114: 4x bilinear upsampling of conv4_3, and the
        // 256 -> 1 bottleneck of the RPN (rpn_model.py:251-267) on the upsampled map
        const Buffer& c4 = ex->buf[C4C];
        const long long n_pix = (long long)p.frames * ex->out_h * ex->out_w;
        constexpr int kLpp = 64;   // 256 channels / 4
        hipLaunchKernelGGL(upsample_bilinear_cb8_kernel<kLpp>,
                           dim3((unsigned)((n_pix * kLpp + 255) / 256)), dim3(256), 0, s, p.map[C4C],
                           c4.H, c4.W, (long long)c4.frame_floats(), ex->out_h, ex->out_w,
                           p.frames, d_feat_out, ex->d_bneck_w, ex->bneck_scale, ex->bneck_shift,
                           d_bottleneck_out);
        DODT_LAUNCH_CHECK();
        return DODT_OK;
    }
    for (int id = UPCONV3; id < FUSION1; ++id)
        if ((rc = run_layer(ex, p, ls[id], nullptr, 0, 0))) return rc;
    // last layer writes straight into the caller's buffer, pad rows sliced off
    // ... and, fused into its epilogue, the 1x1 bottleneck (dt_rpn_model.py:298-322)
    const Layer& last = ls[FUSION1];
    const bool fuse = d_bottleneck_out && bneck_fused(last);
    if ((rc = run_layer(ex, p, last, d_feat_out, ex->pad_top, ex->in_h,
                        fuse ? d_bottleneck_out : nullptr)))
        return rc;
    if (d_bottleneck_out && !fuse) {
        const long long n_pix = (long long)p.frames * ex->in_h * ex->in_w;
        hipLaunchKernelGGL(bottleneck32_kernel, dim3((unsigned)((n_pix * 8 + 255) / 256)),
                           dim3(256), 0, s, d_feat_out, n_pix, ex->d_bneck_w, ex->bneck_scale,
                           ex->bneck_shift, d_bottleneck_out);
        DODT_LAUNCH_CHECK();
    }
    return DODT_OK;
}

int dodt::plan_convs(int kind, int in_h, int in_w, int in_c, int pad_top, int batch, int num_cus, ConvPlan& plan) {
    const bool split = (kind & DODT_EXTRACTOR_SPLIT) != 0;
    const bool bf16 = (kind & DODT_EXTRACTOR_BF16) != 0 || split;
    // (the bf16 kernels have no quarter-size instantiations: single launches)
    const bool shared_gpu = (kind & DODT_EXTRACTOR_SHARED_GPU) != 0 || bf16;
    kind &= ~(DODT_EXTRACTOR_SHARED_GPU | DODT_EXTRACTOR_BF16 | DODT_EXTRACTOR_SPLIT);
    DODT_REQUIRE(kind == DODT_EXTRACTOR_VGG_PYR || kind == DODT_EXTRACTOR_VGG,
                 "dodt_extractor_create: unknown kind %d", kind);
    const bool plain = kind == DODT_EXTRACTOR_VGG;
    DODT_REQUIRE(in_h > 0 && in_w > 0 && in_c >= 2 && in_c % 2 == 0 && pad_top >= 0 && batch >= 1,
                 "dodt_extractor_create: bad sizes (in_c must be even)");
    const int H = in_h + pad_top, W = in_w;
    if (plain) {
        DODT_REQUIRE(!bf16, "dodt_extractor_create: the plain VGG extractor is fp32 only");
        DODT_REQUIRE(pad_top == 0 && H >= 16 && W >= 16,
                     "dodt_extractor_create: plain VGG takes no top padding and >= 16x16 inputs");
    } else {
        DODT_REQUIRE(H % 8 == 0 && W % 8 == 0,
                     "dodt_extractor_create: padded input %dx%d must be divisible by 8 "
                     "(three 2x2 pools, three stride-2 upconvs)", H, W);
    }
    DODT_REQUIRE(num_cus >= 1, "dodt_extractor_create: bad CU count %d", num_cus);
    plan = ConvPlan();
    plan.kind = kind;
    plan.bf16 = bf16;
    plan.parts = split ? 2 : 1;
    plan.H = H; plan.W = W;
    // VALID 2x2 pools floor odd sizes (plain VGG: 175 -> 87, 795 -> 397 -> 198)
    const int H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2, H8 = H4 / 2, W8 = W4 / 2;

    // (LayerId names the layers by their place in this order)
    bool in_order = true;
    auto add = [&](LayerId id, const char* name, bool deconv, int h, int w, int cin, int cout, int src,
                   int src_coff, int dst, int dst_coff, int pool = -1) {
        in_order = in_order && id == (int)plan.layers.size() && deconv == ft::transposed(id);
        Layer l;
        l.pool = pool;
        l.name = name; l.deconv = deconv; l.H = h; l.W = w; l.Cin = cin; l.Cout = cout;
        l.src = src; l.src_coff = src_coff; l.dst = dst; l.dst_coff = dst_coff;
        l.variant = pick_variant(LayerShape{deconv, h, w, cin, cout, bf16, plan.parts, batch, num_cus});
        l.real_cin = cin;
        plan.layers.push_back(l);
    };
    add(CONV1_1, "conv1_1", false, H, W, in_c, 32, X0, 0, C1A, 0);
    add(CONV1_2, "conv1_2", false, H, W, 32, 32, C1A, 0, CAT1, 0, P1);
    add(CONV2_1, "conv2_1", false, H2, W2, 32, 64, P1, 0, C2A, 0);
    add(CONV2_2, "conv2_2", false, H2, W2, 64, 64, C2A, 0, CAT2, 0, P2);
    add(CONV3_1, "conv3_1", false, H4, W4, 64, 128, P2, 0, C3A, 0);
    add(CONV3_2, "conv3_2", false, H4, W4, 128, 128, C3A, 0, C3B, 0);
    add(CONV3_3, "conv3_3", false, H4, W4, 128, 128, C3B, 0, CAT3, 0, P3);
    add(CONV4_1, "conv4_1", false, H8, W8, 128, 256, P3, 0, C4A, 0);
    add(CONV4_2, "conv4_2", false, H8, W8, 256, 256, C4A, 0, C4B, 0);
    add(CONV4_3, "conv4_3", false, H8, W8, 256, 256, C4B, 0, C4C, 0);
    if (!plain) {
        add(UPCONV3, "upconv3", true, H8, W8, 256, 128, C4C, 0, CAT3, 128);
        add(FUSION3, "pyramid_fusion3", false, H4, W4, 256, 64, CAT3, 0, F3, 0);
        add(UPCONV2, "upconv2", true, H4, W4, 64, 64, F3, 0, CAT2, 64);
        add(FUSION2, "pyramid_fusion2", false, H2, W2, 128, 32, CAT2, 0, F2, 0);
        add(UPCONV1, "upconv1", true, H2, W2, 32, 32, F2, 0, CAT1, 32);
        add(FUSION1, "pyramid_fusion1", false, H, W, 64, 32, CAT1, 0, F1, 0);
    }
    if (!in_order) {
        dodt::set_error("dodt_extractor_create: the layers are not in LayerId's order");
        return DODT_ERR_INVALID;
    }
    for (const Layer& l : plan.layers) {
        if (l.variant < 0) {
            dodt::set_error("dodt_extractor_create: no kernel variant for layer %s (%dx%d %d->%d)",
                            l.name.c_str(), l.H, l.W, l.Cin, l.Cout);
            return DODT_ERR_UNSUPPORTED;
        }
    }
    for (Layer& l : plan.layers) {
        plan_layer(l, batch, num_cus, !shared_gpu, l.main.h_items, l.tail.h_items);
        l.main.n_items = (int)l.main.h_items.size();
        l.tail.n_items = (int)l.tail.h_items.size();
    }
    {
        // bf16 conv path: conv1_1 folded into conv1_2's launch when conv1_2 runs on the streaming kernel (same tiles, same
        // weight blocking) and the input rows are whole 16-byte slots (DODT_CONV_BF16_FIRST2=0: two launches)
        const Layer& c11 = plan.layers[CONV1_1];
        const Layer& c12 = plan.layers[CONV1_2];
        const auto& vs = variants();
        // (the input buffer holds exactly conv1_1's in_c channels)
        const KernelVariant& v12 = vs[c12.variant];
        if (conv_switches().bf16_first2 && bf16 && plan.parts == 1 && v12.family == Family::Bf16Stream &&
            v12.stream_nch == 2 && c12.tail.n_items == 0 &&
            c11.Cout == 32 && c11.src_coff == 0 && (W * c11.Cin * 4) % 16 == 0 &&
            variant_can_pool(v12))
            for (size_t i = 0; i < vs.size() && plan.first2_variant < 0; ++i)
                if (vs[i].family == Family::Bf16First2 && vs[i].first2_cin == c11.Cin && vs[i].TH == v12.TH &&
                    vs[i].TW == v12.TW)
                    plan.first2_variant = (int)i;
    }
    return DODT_OK;
}

namespace {

// one layer of a plan as the C ABI reports it (dodt_conv_plan_host, dodt_extractor_layer_plan)
void report_layer(const std::vector<Layer>& layers, int first2_variant, int num_cus, size_t i, dodt_conv_layer_plan* o) {
    const Layer& l = layers[i];
    const bool folding = first2_variant >= 0;
    memset(o, 0, sizeof(*o));
    snprintf(o->name, sizeof(o->name), "%s", l.name.c_str());
    o->h = l.H; o->w = l.W; o->cin = l.Cin; o->cout = l.Cout;
    o->variant[0] = l.main.variant;
    o->variant[1] = l.tail.n_items > 0 ? l.tail.variant : -1;
    o->items[0] = l.main.n_items;
    o->items[1] = l.tail.n_items;
    if (folding && i == CONV1_1) {          // no launch of its own
        o->variant[0] = -1;
        o->items[0] = 0;
        o->folded = 1;
    }
    if (folding && i == CONV1_2) o->variant[0] = first2_variant;   // conv1_2's items, the folding kernel
    for (int j = 0; j < 2; ++j)
        o->grid[j] = o->variant[j] >= 0 ? launch_grid(variants()[o->variant[j]], o->items[j], num_cus) : 0;
    o->pool_fused = l.pool >= 0 && ((folding && i == CONV1_2) || fused_pool_buffer(l) >= 0);
    o->bneck_fused = i == FUSION1 && bneck_fused(l);
}

int report_plan(const std::vector<Layer>& layers, int first2_variant, int num_cus, dodt_conv_layer_plan* out, int n_out,
                int* n_layers) {
    if (n_layers) *n_layers = (int)layers.size();
    if (!out) return DODT_OK;
    DODT_REQUIRE(n_out >= (int)layers.size(), "conv plan: room for %d layers, the net has %d", n_out, (int)layers.size());
    for (size_t i = 0; i < layers.size(); ++i) report_layer(layers, first2_variant, num_cus, i, out + i);
    return DODT_OK;
}

}  // namespace

extern "C" {

int dodt_conv_plan_host(int kind, int in_h, int in_w, int in_c, int pad_top, int batch, int num_cus,
                        dodt_conv_layer_plan* out, int n_out, int* n_layers) {
    ConvPlan plan;
    const int rc = plan_convs(kind, in_h, in_w, in_c, pad_top, batch, num_cus, plan);
    return rc ? rc : report_plan(plan.layers, plan.first2_variant, num_cus, out, n_out, n_layers);
}

int dodt_extractor_layer_plan(const dodt_extractor* ex, dodt_conv_layer_plan* out, int n_out, int* n_layers) {
    DODT_REQUIRE(ex, "dodt_extractor_layer_plan: extractor is NULL");
    return report_plan(ex->layers, ex->first2_variant, ex->num_cus, out, n_out, n_layers);
}

int dodt_conv_variant_count(void) { return (int)variants().size(); }

int dodt_conv_variant_info(int i, dodt_conv_variant* out) {
    DODT_REQUIRE(out && i >= 0 && i < (int)variants().size(), "dodt_conv_variant_info: bad argument");
    const KernelVariant& v = variants()[i];
    memset(out, 0, sizeof(*out));
    out->tw = v.TW; out->th = v.TH; out->bn = v.BN; out->ck = v.CK;
    out->blocks_per_cu = v.blocks_per_cu;
    int family_flags = 0;
    switch (v.family) {
        case Family::Direct: break;
        case Family::SmallCin: family_flags = DODT_VARIANT_SMALL_CIN; break;
        case Family::Wino22: family_flags = DODT_VARIANT_WINO; break;
        case Family::Wino43: family_flags = DODT_VARIANT_WINO | DODT_VARIANT_WINO43; break;
        case Family::DeconvDma: family_flags = DODT_VARIANT_DECONV_DMA; break;
        case Family::Bf16Dma: family_flags = DODT_VARIANT_DMA; break;
        case Family::Bf16Stream: family_flags = DODT_VARIANT_DMA | DODT_VARIANT_STREAM; break;
        case Family::Bf16First2: family_flags = DODT_VARIANT_DMA | DODT_VARIANT_FIRST2; break;
    }
    out->flags = family_flags | (v.deconv ? DODT_VARIANT_DECONV : 0) | (v.tail_only ? DODT_VARIANT_TAIL_ONLY : 0) |
                 (v.bf16 ? DODT_VARIANT_BF16 : 0) | (v.parts == 2 ? DODT_VARIANT_SPLIT : 0) |
                 (variant_xcd_queue(v) ? DODT_VARIANT_XCD_QUEUE : 0) | (variant_can_pool(v) ? DODT_VARIANT_CAN_POOL : 0);
    out->lds_bytes = v.lds_bytes;
    snprintf(out->kernel, sizeof(out->kernel), "%s", kernel_name(v));
    return DODT_OK;
}

int dodt_extractor_create(dodt_ctx* ctx, int kind, int in_h, int in_w, int in_c, int pad_top,
                          int batch, dodt_extractor** out) {
    DODT_REQUIRE(ctx && out, "dodt_extractor_create: NULL argument");
    const int num_cus = ctx->plan_cus > 0 ? ctx->plan_cus : ctx->num_cus;
    ConvPlan plan;
    {
        const int rc = plan_convs(kind, in_h, in_w, in_c, pad_top, batch, num_cus, plan);
        if (rc) return rc;
    }
    kind = plan.kind;
    const bool plain = kind == DODT_EXTRACTOR_VGG;
    const bool bf16 = plan.bf16;
    const int H = plan.H, W = plan.W;
    for (const KernelVariant& v : variants()) DODT_HIP_CHECK(v.prepare());

    dodt_extractor* ex = new dodt_extractor();
    ex->num_cus = num_cus;
    ex->ctx = ctx;
    ex->kind = kind;
    ex->in_h = in_h; ex->in_w = in_w; ex->in_c = in_c; ex->pad_top = pad_top; ex->batch = batch;
    ex->H = H; ex->W = W;
    ex->bf16 = bf16;
    ex->parts = plan.parts;
    auto setb = [&](int id, int h, int w, int c) { ex->buf[id].H = h; ex->buf[id].W = w; ex->buf[id].C = c; };
    // VALID 2x2 pools floor odd sizes (plain VGG: 175 -> 87, 795 -> 397 -> 198)
    const int H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2, H8 = H4 / 2, W8 = W4 / 2;
    setb(X0, H, W, in_c);
    setb(C1A, H, W, 32); setb(CAT1, H, W, plain ? 32 : 64); setb(P1, H2, W2, 32);
    setb(C2A, H2, W2, 64); setb(CAT2, H2, W2, plain ? 64 : 128); setb(P2, H4, W4, 64);
    setb(C3A, H4, W4, 128); setb(C3B, H4, W4, 128); setb(CAT3, H4, W4, plain ? 128 : 256);
    setb(P3, H8, W8, 128);
    setb(C4A, H8, W8, 256); setb(C4B, H8, W8, 256); setb(C4C, H8, W8, 256);
    if (!plain) { setb(F3, H4, W4, 64); setb(F2, H2, W2, 32); setb(F1, H, W, 32); }
    if (plain) {
        // bev_vgg.py:102-112: resize_bilinear to input_pixel_size / 8 * upsampling_multiplier (4),
        // a float pair that TF casts to int32 (350 x 400 for 700 x 800, 240 x 795 for 480 x 1590)
        ex->out_h = (int)((double)in_h / 8.0 * 4.0);
        ex->out_w = (int)((double)in_w / 8.0 * 4.0);
        ex->out_c = 256;
    } else {
        ex->out_h = in_h; ex->out_w = in_w; ex->out_c = 32;
    }
    for (int i = 0; i < NBUF; ++i) {
        ex->buf[i].bf16 = bf16 && i != X0 && i != F1;
        ex->buf[i].parts = ex->buf[i].bf16 ? ex->parts : 1;
    }
    for (int i = 0; i < NBUF; ++i) {
        if (i == F1 || ex->buf[i].H == 0) continue;  // F1: written into the caller's buffer
        const size_t bytes = ex->buf[i].frame_floats() * batch * ex->buf[i].parts * sizeof(float);
        hipError_t e = hipMalloc(&ex->buf[i].ptr, bytes);
        if (e != hipSuccess) {
            dodt::set_error("dodt_extractor_create: hipMalloc(%zu) failed: %s", bytes,
                            hipGetErrorString(e));
            dodt_extractor_destroy(ex);
            return DODT_ERR_HIP;
        }
    }
    DODT_HIP_CHECK(hipMalloc(&ex->d_counters, 4096 * sizeof(int)));
    DODT_HIP_CHECK(hipMemsetAsync(ex->d_counters, 0, 4096 * sizeof(int), ctx->stream));
    DODT_HIP_CHECK(hipMalloc(&ex->d_zeros, 256));
    DODT_HIP_CHECK(hipMemsetAsync(ex->d_zeros, 0, 256, ctx->stream));
    // the pad rows of X0 stay zero for the life of the extractor
    DODT_HIP_CHECK(hipMemsetAsync(ex->buf[X0].ptr, 0,
                                  ex->buf[X0].frame_floats() * batch * sizeof(float), ctx->stream));

    // the plan's layers; their item tables go to the device
    ex->layers = std::move(plan.layers);
    ex->first2_variant = plan.first2_variant;
    for (Layer& l : ex->layers) {
        for (Launch* ln : {&l.main, &l.tail}) {
            if (ln->h_items.empty()) continue;
            DODT_HIP_CHECK(hipMalloc(&ln->d_items, ln->h_items.size() * sizeof(int4)));
            DODT_HIP_CHECK(hipMemcpyAsync(ln->d_items, ln->h_items.data(), ln->h_items.size() * sizeof(int4),
                                          hipMemcpyHostToDevice, ctx->stream));
        }
    }
    DODT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (conv_switches().debug_plan) {
        if (ex->first2_variant >= 0) fprintf(stderr, "[dodt] conv1_1 runs folded into conv1_2's launch\n");
        for (const Layer& l : ex->layers) {
            const KernelVariant& v = variants()[l.variant];
            fprintf(stderr, "[dodt] %-16s %4dx%-4d %3d->%-3d TW%d TH%d BN%d CK%d lds %d items %d",
                    l.name.c_str(), l.H, l.W, l.Cin, l.Cout, v.TW, v.TH, v.BN, v.CK, v.lds_bytes,
                    l.main.n_items);
            if (l.tail.n_items) {
                const KernelVariant& c = variants()[l.tail.variant];
                fprintf(stderr, " + tail TH%d BN%d items %d", c.TH, c.BN, l.tail.n_items);
            }
            fprintf(stderr, "\n");
        }
    }
    *out = ex;
    return DODT_OK;
}

int dodt_extractor_destroy(dodt_extractor* ex) {
    if (!ex) return DODT_OK;
    if (ex->ctx) (void)hipStreamSynchronize(ex->ctx->stream);
    if (ex->own_x0) ex->buf[X0].ptr = ex->own_x0;      // (dodt_extractor_set_input: never free a caller's input buffer)
    free_frame_tables(ex);
    for (int i = 0; i < NBUF; ++i)
        if (ex->buf[i].ptr) (void)hipFree(ex->buf[i].ptr);
    for (Layer& l : ex->layers) {
        for (Launch* ln : {&l.main, &l.tail}) {
            if (ln->d_w) (void)hipFree(ln->d_w);
            if (ln->d_items) (void)hipFree(ln->d_items);
            if (ln->d_skip) (void)hipFree(ln->d_skip);
        }
        if (l.d_scale) (void)hipFree(l.d_scale);
        if (l.d_shift) (void)hipFree(l.d_shift);
        if (l.d_first_w) (void)hipFree(l.d_first_w);
    }
    if (ex->d_bneck_w) (void)hipFree(ex->d_bneck_w);
    for (Layer& l : ex->layers) {
        if (l.ev0) (void)hipEventDestroy(l.ev0);
        if (l.ev1) (void)hipEventDestroy(l.ev1);
    }
    if (ex->d_counters) (void)hipFree(ex->d_counters);
    if (ex->d_zeros) (void)hipFree(ex->d_zeros);
    delete ex;
    return DODT_OK;
}

int dodt_extractor_set_layer(dodt_extractor* ex, const char* name, const float* w, int kh, int kw,
                             int c_a, int c_b, const float* beta, const float* mean,
                             const float* var) {
    DODT_REQUIRE(ex && name && w && beta && mean && var, "dodt_extractor_set_layer: NULL argument");
    hipStream_t s = ex->ctx->stream;
    int rc;
    // new weights: the input-independent outputs the skip tables leave alone change (the next forward primes)
    ex->primed = false;
    forget_pairs(ex);
    ex->store_valid = false;
    if (std::strcmp(name, "bottleneck") == 0) {
        const int fc = ex->out_c;   // 32 (pyramid) or 256 (plain VGG: rpn_model.py:251-267)
        DODT_REQUIRE(kh == 1 && kw == 1 && c_a == fc && c_b == 1,
                     "bottleneck must be (1,1,%d,1), got (%d,%d,%d,%d)", fc, kh, kw, c_a, c_b);
        if ((rc = upload(&ex->d_bneck_w, std::vector<float>(w, w + fc), s))) return rc;
        const float inv = 1.0f / std::sqrt(var[0] + 0.001f);
        ex->bneck_scale = inv;
        ex->bneck_shift = beta[0] - mean[0] * inv;
        ex->bneck_loaded = true;
        return DODT_OK;
    }
    const int li = find_layer(ex, name);
    DODT_REQUIRE(li >= 0, "dodt_extractor_set_layer: unknown layer '%s'", name);
    Layer& l = ex->layers[li];
    DODT_REQUIRE(kh == 3 && kw == 3, "layer %s: kernel must be 3x3", name);
    // TF layouts: conv2d (kh,kw,cin,cout); conv2d_transpose (kh,kw,cout,cin)
    const int cin = l.deconv ? c_b : c_a, cout = l.deconv ? c_a : c_b;
    DODT_REQUIRE(cout == l.Cout && cin <= l.Cin && (cin == l.Cin || li == 0),
                 "layer %s: expected %d->%d channels, got %d->%d", name, l.Cin, l.Cout, cin, cout);
    for (Launch* ln : {&l.main, &l.tail}) {
        if (ln->variant < 0) continue;
        if (ln == &l.tail && variants()[l.tail.variant].BN == variants()[l.main.variant].BN) {
            ln->d_w = nullptr;   // same blocking: run_launch takes the main launch's copy
            continue;
        }
        const KernelVariant& v = variants()[ln->variant];
        const WeightTile t{v.BN, v.CK, v.bf16, v.family == Family::SmallCin, v.parts};
        const std::vector<float> blocked = v.family == Family::DeconvDma ? block_deconv_dma(t, l, w, cin, cout)
                                           : v.family == Family::Wino43  ? block_wino43(t, l, w, cin, cout)
                                           : v.family == Family::Wino22  ? block_wino22(t, l, w, cin, cout)
                                                                         : block_direct(t, l, w, cin, cout);
        if ((rc = upload(&ln->d_w, blocked, s))) return rc;
    }
    if (li == 0 && ex->bf16 && ex->parts == 1 && l.Cout == 32 && (l.Cin == 6 || l.Cin == 4))
        if ((rc = upload(reinterpret_cast<uint16_t**>(&l.d_first_w), pack_first2(l, w, cin, cout), s))) return rc;
    std::vector<float> scale(l.Cout), shift(l.Cout);
    for (int co = 0; co < l.Cout; ++co) {
        const float inv = 1.0f / std::sqrt(var[co] + 0.001f);
        scale[co] = inv;
        shift[co] = beta[co] - mean[co] * inv;
    }
    if ((rc = upload(&l.d_scale, scale, s)) || (rc = upload(&l.d_shift, shift, s))) return rc;
    l.loaded = true;
    l.real_cin = cin;
    return DODT_OK;
}

int dodt_extractor_input(dodt_extractor* ex, float** d_ptr, long long* frame_stride_floats) {
    DODT_REQUIRE(ex && d_ptr && frame_stride_floats, "dodt_extractor_input: NULL argument");
    const Buffer& x0 = ex->buf[X0];
    *d_ptr = x0.ptr + (size_t)ex->pad_top * x0.W * x0.C;
    *frame_stride_floats = (long long)x0.frame_floats();
    return DODT_OK;
}

int dodt_extractor_forward(dodt_extractor* ex, const float* d_in, float* d_feat_out,
                           float* d_bottleneck_out) {
    return forward(ex, d_in, nullptr, d_feat_out, d_bottleneck_out, false);
}

int dodt_extractor_forward_padded(dodt_extractor* ex, const float* d_x0, float* d_feat_out,
                                  float* d_bottleneck_out) {
    DODT_REQUIRE(ex && d_x0 && d_feat_out, "dodt_extractor_forward_padded: NULL argument");
    // the first layer reads the caller's buffer in place of the extractor's own input buffer
    return forward(ex, nullptr, d_x0, d_feat_out, d_bottleneck_out, false);
}

int dodt_extractor_set_input(dodt_extractor* ex, const float* d_x0) {
    DODT_REQUIRE(ex, "dodt_extractor_set_input: extractor is NULL");
    if (!ex->own_x0) ex->own_x0 = ex->buf[X0].ptr;
    ex->buf[X0].ptr = d_x0 ? const_cast<float*>(d_x0) : ex->own_x0;
    return DODT_OK;
}

}  // extern "C"

namespace {

int forward(dodt_extractor* ex, const float* d_in, const float* d_x0, float* d_feat_out, float* d_bottleneck_out,
            bool timed) {
    DODT_REQUIRE(ex && d_feat_out, "dodt_extractor_forward: NULL argument");
    for (const Layer& l : ex->layers)
        DODT_REQUIRE(l.loaded, "dodt_extractor_forward: weights of layer %s not set",
                     l.name.c_str());
    DODT_REQUIRE(!d_bottleneck_out || ex->bneck_loaded,
                 "dodt_extractor_forward: bottleneck weights not set");
    hipStream_t s = ex->ctx->stream;
    Pass p;
    for (int i = 0; i < NBUF; ++i) p.map[i] = ex->buf[i].ptr;
    if (d_x0) p.map[X0] = const_cast<float*>(d_x0);
    p.frames = ex->batch;
    p.timed = timed;
    const Buffer& x0 = ex->buf[X0];
    float* own_in = p.map[X0] + (size_t)ex->pad_top * x0.W * x0.C;
    if (d_in && d_in != own_in) {
        const long long n4 = (long long)ex->in_h * ex->in_w * ex->in_c / 4;
        DODT_REQUIRE(((long long)ex->in_h * ex->in_w * ex->in_c) % 4 == 0, "input not float4-sized");
        hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)((n4 * ex->batch + 255) / 256)),
                           dim3(256), 0, s, reinterpret_cast<const float4*>(d_in),
                           reinterpret_cast<float4*>(own_in), n4, n4,
                           (long long)x0.frame_floats() / 4, ex->batch);
        DODT_LAUNCH_CHECK();
    }
    // (the whole block: the launches' counters in words 0..63, the XCD-grouped queues' in words 2048..; the
    //  diagnostic words in between are only read right behind the launch that wrote them)
    DODT_HIP_CHECK(hipMemsetAsync(ex->d_counters, 0, 4096 * sizeof(int), s));
    // skip tables once a full forward has primed the buffers; pyramid_fusion1 writes the caller's buffers, so it
    // primes every output pair of its own
    const bool skip = ex->skip_on && ex->primed;
    const int known = find_pair(ex, d_feat_out, d_bottleneck_out);
    const bool last_skip = skip && known >= 0;
    choose_tables(ex, skip, last_skip, p);
    // (per-frame tables: a new pair takes the item set of the pair it evicts, or a free one)
    const int slot = known >= 0 ? ex->pairs[known].slot : slot_for_new_pair(ex);
    int rc;
    if (ex->frame_on && (rc = begin_frame_forward(ex, p, slot, last_skip, d_feat_out, d_bottleneck_out))) return rc;
    if ((rc = run_layers(ex, p, d_feat_out, d_bottleneck_out))) return rc;
    if (ex->skip_on) {
        ex->primed = true;
        if (known < 0) add_pair(ex, d_feat_out, d_bottleneck_out, slot);
    }
    return DODT_OK;
}

}  // namespace

extern "C" {

int dodt_extractor_output_shape(const dodt_extractor* ex, int* h, int* w, int* c) {
    DODT_REQUIRE(ex, "dodt_extractor_output_shape: NULL argument");
    if (h) *h = ex->out_h;
    if (w) *w = ex->out_w;
    if (c) *c = ex->out_c;
    return DODT_OK;
}

int dodt_extractor_first_layers_folded(const dodt_extractor* ex) {
    DODT_REQUIRE(ex, "dodt_extractor_first_layers_folded: extractor is NULL");
    return ex->first2_variant >= 0 ? 1 : 0;
}

int dodt_extractor_read_activation(dodt_extractor* ex, const char* name, float* dst, int* h,
                                   int* w, int* c) {
    DODT_REQUIRE(ex && name, "dodt_extractor_read_activation: NULL argument");
    // "store:<layer>": the constants store's map of the layer (one frame, returned for every frame of the batch);
    // "store:pyramid_fusion1" and "store:bottleneck": the store's output pair
    const bool stored = std::strncmp(name, "store:", 6) == 0;
    if (stored) {
        name += 6;
        DODT_REQUIRE(ex->store_valid, "dodt_extractor_read_activation: no constants store (no forward has restored yet)");
        const bool bn = std::strcmp(name, "bottleneck") == 0;
        if (bn || std::strcmp(name, "pyramid_fusion1") == 0) {
            DODT_REQUIRE(!bn || ex->bneck_loaded, "dodt_extractor_read_activation: the store holds no bottleneck map");
            const int cc = bn ? 1 : ex->out_c;
            if (h) *h = ex->out_h;
            if (w) *w = ex->out_w;
            if (c) *c = cc;
            if (!dst) return DODT_OK;
            const size_t n = (size_t)ex->out_h * ex->out_w * cc;
            for (int f = 0; f < ex->batch; ++f)
                DODT_HIP_CHECK(hipMemcpy(dst + f * n, bn ? ex->store_bneck : ex->store_feat, n * sizeof(float), hipMemcpyDeviceToHost));
            return DODT_OK;
        }
    }
    const int li = find_layer(ex, name);
    DODT_REQUIRE(li >= 0, "dodt_extractor_read_activation: unknown layer '%s'", name);
    const Layer& l = ex->layers[li];
    DODT_REQUIRE(!(li == 0 && ex->first2_variant >= 0),
                 "layer %s runs folded into conv1_2's launch: its map is not stored (DODT_CONV_BF16_FIRST2=0 keeps it)", name);
    Buffer b = ex->buf[l.dst];
    if (stored) b.ptr = ex->store[l.dst];
    const size_t frame_step = stored ? 0 : b.frame_floats();
    DODT_REQUIRE(b.ptr != nullptr,
                 "layer %s is written straight into the caller's output buffer", name);
    const int oh = l.deconv ? 2 * l.H : l.H, ow = l.deconv ? 2 * l.W : l.W;
    if (h) *h = oh;
    if (w) *w = ow;
    if (c) *c = l.Cout;
    if (!dst) return DODT_OK;
    // CB8 fp32 (or CB16 bf16) planes of every frame -> dense NHWC fp32 host tensor
    DODT_HIP_CHECK(hipStreamSynchronize(ex->ctx->stream));
    const int pc = b.bf16 ? 16 : 8;                 // channels per plane
    const size_t plane = (size_t)oh * ow * 8;       // floats per plane, both layouts
    const int planes = l.Cout / pc;
    std::vector<float> tmp(plane * planes);
    const uint16_t* tmp16 = reinterpret_cast<const uint16_t*>(tmp.data());
    for (int f = 0; f < ex->batch; ++f) {
        DODT_HIP_CHECK(hipMemcpy(tmp.data(),
                                 b.ptr + (size_t)f * frame_step + (size_t)(l.dst_coff / pc) * plane,
                                 tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
        float* o = dst + (size_t)f * oh * ow * l.Cout;
        for (int pl = 0; pl < planes; ++pl)
            for (size_t px = 0; px < (size_t)oh * ow; ++px)
                for (int k = 0; k < pc; ++k)
                    o[px * l.Cout + pl * pc + k] =
                        b.bf16 ? dodt::bf16_to_float(tmp16[(pl * plane + px * 8) * 2 + k])
                               : tmp[pl * plane + px * 8 + k];
        if (b.parts == 2) {   // split mode: add the lo map
            DODT_HIP_CHECK(hipMemcpy(tmp.data(),
                                     b.ptr + (size_t)(ex->batch + f) * b.frame_floats() +
                                         (size_t)(l.dst_coff / pc) * plane,
                                     tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (int pl = 0; pl < planes; ++pl)
                for (size_t px = 0; px < (size_t)oh * ow; ++px)
                    for (int k = 0; k < pc; ++k)
                        o[px * l.Cout + pl * pc + k] +=
                            dodt::bf16_to_float(tmp16[(pl * plane + px * 8) * 2 + k]);
        }
    }
    return DODT_OK;
}

double dodt_extractor_bytes(const dodt_extractor* ex) {
    if (!ex) return 0.0;
    double b = 0.0;
    const WorkShare share(ex);
    for (const Layer& l : ex->layers) b += layer_bytes(ex, l, share.of(ex, l)) + share.restore_bytes(ex, l);
    if (ex->kind == DODT_EXTRACTOR_VGG)   // upsampling: conv4_3 read, the feature map written
        b += (double)ex->batch * ((double)ex->buf[C4C].H * ex->buf[C4C].W * 256 +
                                  (double)ex->out_h * ex->out_w * 256) * 4.0;
    b += (double)ex->batch * ex->out_h * ex->out_w * 4.0;   // bottleneck map
    return b;
}

double dodt_extractor_mfma_flops(const dodt_extractor* ex) {
    if (!ex) return 0.0;
    double f = 0.0;
    const WorkShare share(ex);
    for (const Layer& l : ex->layers) f += layer_executed_flops(ex, l, share.of(ex, l));
    return f;
}

int dodt_extractor_layer_count(const dodt_extractor* ex) { return ex ? (int)ex->layers.size() : 0; }

int dodt_extractor_forward_timed(dodt_extractor* ex, const float* d_in, float* d_feat_out,
                                 float* d_bottleneck_out, dodt_layer_info* info, int n_info) {
    DODT_REQUIRE(ex && info && n_info >= (int)ex->layers.size(),
                 "dodt_extractor_forward_timed: info must hold dodt_extractor_layer_count() entries");
    for (Layer& l : ex->layers) {
        if (!l.ev0) DODT_HIP_CHECK(hipEventCreate(&l.ev0));
        if (!l.ev1) DODT_HIP_CHECK(hipEventCreate(&l.ev1));
    }
    const int rc = forward(ex, d_in, nullptr, d_feat_out, d_bottleneck_out, true);
    if (rc) return rc;
    DODT_HIP_CHECK(hipStreamSynchronize(ex->ctx->stream));
    const WorkShare share(ex);
    for (size_t i = 0; i < ex->layers.size(); ++i) {
        const Layer& l = ex->layers[i];
        dodt_layer_info& o = info[i];
        memset(&o, 0, sizeof(o));
        snprintf(o.name, sizeof(o.name), "%s", l.name.c_str());
        const bool folded = ex->first2_variant >= 0 && i < 2;      // conv1_1 and conv1_2 are one launch, timed as conv1_2
        snprintf(o.kernel, sizeof(o.kernel), "%s", kernel_name(variants()[folded ? ex->first2_variant : l.main.variant]));
        // (what this forward ran: choose_tables' record; per-frame tables: the counts the builder wrote)
        const bool pf = share.per_frame(ex, i);
        const double frac = pf ? share.of(ex, l) : ex->ran[i].kind != Tables::Full ? l.skip_frac : 1.0;
        const int n_main = pf ? share.items(i, 0) : ex->ran[i].n[0];
        const int n_tail = pf ? share.items(i, 1) : ex->ran[i].n[1];
        o.launches = folded && i == 0 ? 0 : (n_main > 0) + (n_tail > 0);
        o.items = n_main + n_tail;
        o.flops_direct = layer_direct_flops(ex, l, frac);
        o.flops_executed = layer_executed_flops(ex, l, frac);
        o.bytes = layer_bytes(ex, l, frac);
        DODT_HIP_CHECK(hipEventElapsedTime(&o.ms, l.ev0, l.ev1));
    }
    return DODT_OK;
}

double dodt_extractor_flops(const dodt_extractor* ex) {
    if (!ex) return 0.0;
    double f = 0.0;  // 2*M*N*K per layer; transposed convs counted on input pixels; skipped items not counted
    const WorkShare share(ex);
    for (const Layer& l : ex->layers) f += layer_direct_flops(ex, l, share.of(ex, l));
    return f;
}

}  // extern "C"
