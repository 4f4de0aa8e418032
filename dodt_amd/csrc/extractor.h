// The VGG-pyramid extractor's host-side state, shared by its translation units: conv.hip (variants, lifecycle, the
// forward, accounting), conv_weights.hip (weight blocking) and conv_skip.hip (skip tables, per-frame tables, the
// constants store).  No kernel lives here.
#pragma once
#include <string>
#include <vector>

#include "common.h"
#include "frame_tables.h"

namespace dodt {

struct KernelVariant;   // conv_variants.h

struct Buffer {
    int H = 0, W = 0, C = 0;
    float* ptr = nullptr;
    bool bf16 = false;   // CB16 bf16 map (2 bytes per element) instead of CB8 / NHWC fp32
    int parts = 1;       // 2: split mode, [hi map of all frames | lo map of all frames]
    size_t frame_floats() const { return (size_t)H * W * C / (bf16 ? 2 : 1); }   // one part
};

// one kernel launch of a layer: a variant and the work items it walks
struct Launch {
    int variant = -1;
    int n_items = 0;
    int4* d_items = nullptr;
    float* d_w = nullptr;   // weights blocked for this variant's BN
    std::vector<int4> h_items;   // the full table on the host (skip tables are filtered from it)
    int n_skip = -1;             // >= 0: the skip table (dodt_extractor_set_input_support), possibly empty
    int4* d_skip = nullptr;
    // per-frame tables (dodt_extractor_set_frame_tables): this forward's items of the skip table and their count
    int4* d_run = nullptr;
    int* d_count = nullptr;
};

struct Layer {
    std::string name;
    bool deconv = false;
    int H = 0, W = 0;  // GEMM grid (conv: output size; deconv: input size)
    int Cin = 0, Cout = 0;
    int src = -1, src_coff = 0;
    int dst = -1, dst_coff = 0;
    int pool = -1;       // the buffer the 2x2 max pool behind the layer writes (conv1_2, conv2_2, conv3_3), or -1
    int variant = -1;
    Launch main, tail;   // tail.n_items == 0: single launch
    float *d_scale = nullptr, *d_shift = nullptr;
    bool loaded = false;
    int real_cin = 0;  // channels that carry data (conv1_1 of the image net: 3 of 4)
    float* d_first_w = nullptr;   // conv1_1 of a bf16 extractor: hi + lo bf16 MFMA fragments for conv3x3_bf16_first2_kernel
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // dodt_extractor_forward_timed
    double skip_frac = 1.0;   // share of the layer's MFMA work its skip tables keep
};

enum Buf { X0, C1A, CAT1, P1, C2A, CAT2, P2, C3A, C3B, CAT3, P3, C4A, C4B, C4C, F3, F2, F1, NBUF };

// the layers in launch order, as dodt_extractor_create adds them (the plain VGG net ends behind CONV4_3)
enum LayerId {
    CONV1_1, CONV1_2, CONV2_1, CONV2_2, CONV3_1, CONV3_2, CONV3_3, CONV4_1, CONV4_2, CONV4_3,
    UPCONV3, FUSION3, UPCONV2, FUSION2, UPCONV1, FUSION1, NLAYERS
};
static_assert(NLAYERS == ft::kLayers, "the per-frame builder walks the pyramid net's layers");
static_assert(ft::transposed(UPCONV3) && ft::transposed(UPCONV2) && ft::transposed(UPCONV1) && !ft::transposed(FUSION1) &&
                  !ft::transposed(CONV4_3), "the per-frame builder's transposed convs are the net's");

// which item tables a layer's launches walk
enum class Tables { Full, Static, PerFrame };

struct ItemTable {
    const int4* items = nullptr;
    int n = 0;                   // items (per-frame tables: the most there can be; the grid is sized by it)
    const int* n_dev = nullptr;  // per-frame tables: how many of them this forward runs, on the device
    bool dense = false;          // every tile of every frame in index order (the first-layer kernel needs no table then)
};

// One walk over the layers (run_layers): where each map lives, how many frames, what every launch walks.
struct Pass {
    float* map[NBUF] = {};
    int frames = 0;
    bool timed = false;          // an event pair around every layer (Layer::ev0, ev1)
    ItemTable table[NLAYERS][2]; // [layer][main, tail]
};

// an output pair pyramid_fusion1 has written with full tables since the last weight load, and which of the eight
// item sets of its last forward into the pair (per-frame tables) is the pair's
struct OutPair {
    const float* feat = nullptr;
    const float* bneck = nullptr;
    int slot = 0;
};
constexpr int kOutPairs = 8;

// What the host decides about an extractor before it touches the device (plan_convs): the layers in launch order,
// each with its variants and the item tables of its launches (Launch::h_items), and the first layers' folding.
struct ConvPlan {
    int kind = DODT_EXTRACTOR_VGG_PYR;   // without the flag bits
    bool bf16 = false;
    int parts = 1;
    int H = 0, W = 0;            // padded input size
    std::vector<Layer> layers;
    int first2_variant = -1;     // dodt_extractor::first2_variant
};

}  // namespace dodt

struct dodt_extractor {
    dodt_ctx* ctx = nullptr;
    int in_h = 0, in_w = 0, in_c = 0, pad_top = 0, batch = 0;
    int kind = DODT_EXTRACTOR_VGG_PYR;
    int out_h = 0, out_w = 0, out_c = 32;   // the returned feature map
    bool bf16 = false;  // conv path on bf16 MFMA (fp32 accumulate, fp32 BN/ReLU, bf16 maps)
    int parts = 1;      // 2: split mode (hi + lo bf16 maps and weights, three MFMAs per term)
    int H = 0, W = 0;  // padded input size
    int num_cus = 0;   // CUs the layers were planned for and the grids are sized by (dodt_ctx_set_plan_cus, or the device's)
    dodt::Buffer buf[dodt::NBUF];
    std::vector<dodt::Layer> layers;
    float* d_bneck_w = nullptr;
    int* d_counters = nullptr;  // two work-item counters per layer, zeroed every forward
    float* d_zeros = nullptr;   // a zero page (Winograd kernel: out-of-image pixels)
    float bneck_scale = 1.0f, bneck_shift = 0.0f;
    bool bneck_loaded = false;
    double flops = 0.0;
    int first2_variant = -1;   // >= 0: conv1_1 runs folded into conv1_2's launch (bf16 conv path; DODT_CONV_BF16_FIRST2=0: not)
    float* own_x0 = nullptr;   // the extractor's own input buffer while dodt_extractor_set_input points X0 elsewhere
    // input support (dodt_extractor_set_input_support): skip tables built; a full forward has run since the last
    // weight load; the output pairs written with full tables since then, oldest first
    bool skip_on = false;
    bool primed = false;
    dodt::OutPair pairs[dodt::kOutPairs];
    int n_pairs = 0;
    // what the last forward ran (choose_tables): per layer the kind of table and the host's item count per launch
    struct Ran {
        dodt::Tables kind = dodt::Tables::Full;
        int n[2] = {0, 0};
    } ran[dodt::NLAYERS];
    bool restoring = false;   // the last forward ran the restore launch
    // per-frame tables (dodt_extractor_set_frame_tables): the builder's plan (frame_tables.h), its device copy, the
    // frames' input bit masks, every allocation of the tables, and pyramid_fusion1's item set per OutPair::slot
    bool frame_on = false;
    dodt::ft::Plan frame_plan;
    dodt::ft::Plan* d_frame_plan = nullptr;
    uint32_t* d_frame_bits = nullptr;
    int* d_frame_counts = nullptr;
    std::vector<void*> frame_allocs;
    uint8_t* out_prev[dodt::kOutPairs][2] = {};
    // constants store (per-frame tables): one frame of every layer buffer and of the (feature, bottleneck) pair as a
    // forward on zeros writes them -- what an output holds that no input reaches.  Taken by the first forward that
    // restores from it (take_store), again after new weights; freed with the per-frame tables.
    float* store[dodt::NBUF] = {};
    float* store_feat = nullptr;
    float* store_bneck = nullptr;
    dodt::ft::RestorePlan* d_restore_plan = nullptr;
    bool store_valid = false;
    size_t store_bytes = 0;
};

namespace dodt {

// --- conv.hip ---
const std::vector<KernelVariant>& variants();
// the buffer a layer's epilogue pools into (Layer::pool where the tiling allows), or -1
int fused_pool_buffer(const Layer& l);
// pyramid_fusion1 computes the 1x1 bottleneck in its epilogue (32-channel tiles)
bool bneck_fused(const Layer& last);
// The layer list of an extractor of `kind` (flag bits included) for num_cus CUs: each layer's variant, its main and
// tail launch with their item tables, the folded first layers.  Host only: reads no device and allocates nothing on one.
int plan_convs(int kind, int in_h, int in_w, int in_c, int pad_top, int batch, int num_cus, ConvPlan& plan);
// the layers of one walk on the extractor's stream; writes nothing in the extractor
int run_layers(const dodt_extractor* ex, const Pass& p, float* d_feat_out, float* d_bottleneck_out);

// --- conv_weights.hip: TF-layout weights (kh, kw, cin, cout; transposed convs kh, kw, cout, cin) -> a variant's blocking
struct WeightTile {   // what the blocking depends on of a KernelVariant
    int BN, CK;
    bool bf16, small_cin;
    int parts;
};
std::vector<float> block_deconv_dma(const WeightTile& v, const Layer& l, const float* w, int cin, int cout);
std::vector<float> block_wino43(const WeightTile& v, const Layer& l, const float* w, int cin, int cout);
std::vector<float> block_wino22(const WeightTile& v, const Layer& l, const float* w, int cin, int cout);
std::vector<float> block_direct(const WeightTile& v, const Layer& l, const float* w, int cin, int cout);
std::vector<uint16_t> pack_first2(const Layer& l, const float* w, int cin, int cout);
// a host vector to *d (allocated when null) on the stream; returns once the copy is done
template <class T>
int upload(T** d, const std::vector<T>& h, hipStream_t s) {
    if (!*d) DODT_HIP_CHECK(hipMalloc(d, h.size() * sizeof(T)));
    DODT_HIP_CHECK(hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
    DODT_HIP_CHECK(hipStreamSynchronize(s));
    return DODT_OK;
}

// --- conv_skip.hip ---
void free_frame_tables(dodt_extractor* ex);
// the remembered output pairs: index of a pair or -1; the item-set slot a new pair takes (the one of the pair it
// evicts, or the lowest free one); forget all; remember a pair behind the others, evicting the oldest of eight
int find_pair(const dodt_extractor* ex, const float* feat, const float* bneck);
int slot_for_new_pair(const dodt_extractor* ex);
void forget_pairs(dodt_extractor* ex);
void add_pair(dodt_extractor* ex, const float* feat, const float* bneck, int slot);
// Which table every launch of a forward walks: skip: the layers ahead of pyramid_fusion1 take their skip tables,
// last_skip: pyramid_fusion1 too.  Writes the pass and the extractor's record of the forward (ran, restoring).
void choose_tables(dodt_extractor* ex, bool skip, bool last_skip, Pass& p);
// per-frame tables, ahead of conv1_1: the store where a restoring forward finds none, the builder, the restore launch
int begin_frame_forward(dodt_extractor* ex, const Pass& p, int slot, bool last_skip, float* d_feat_out,
                        float* d_bottleneck_out);

// the share of a layer's work a forward in steady state runs (skip tables once primed)
inline double steady_frac(const dodt_extractor* ex, const Layer& l) { return ex->skip_on ? l.skip_frac : 1.0; }

// The share of a layer's work that is counted: the steady state's (steady_frac), or with per-frame tables what the
// last finished forward ran of a layer that took them (waits for the stream).
struct WorkShare {
    int counts[2 * ft::kTables];   // computed items per table, then restored items per table
    bool have;
    explicit WorkShare(const dodt_extractor* ex);
    bool per_frame(const dodt_extractor* ex, size_t li) const {
        return have && li < (size_t)NLAYERS && ex->ran[li].kind == Tables::PerFrame;
    }
    int items(size_t li, int j) const { return counts[2 * li + j]; }
    // the items of the launch whose outputs the forward copied back from the store (none where a full table ran)
    int restored(const dodt_extractor* ex, size_t li, int j) const {
        return per_frame(ex, li) && ex->restoring ? counts[ft::kTables + 2 * li + j] : 0;
    }
    double restore_bytes(const dodt_extractor* ex, const Layer& l) const;
    double of(const dodt_extractor* ex, const Layer& l) const;
};

}  // namespace dodt
