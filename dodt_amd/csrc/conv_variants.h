// Kernel-variant table entries of the conv kernels (shared by conv.hip, which instantiates
// the fp32 kernels, and conv_bf16.hip, which instantiates the bf16 ones).
#pragma once
#include <vector>

#include "conv_kernels.h"
#include "wino_kernels.h"
#include "wino43_kernel.h"
#include "deconv_kernel.h"
#include "conv_bf16_dma.h"

namespace dodt {

// Which __global__ template a variant launches, and with it its queue code, weight blocking and planning rule.
enum class Family {
    Direct,      // the register-staged template (conv_kernels.h): conv and transposed conv; fp32, bf16 and split
    SmallCin,    // the first layer's kernel (conv_kernels.h): 4 / 6 input channels
    Wino22,      // fp32 Winograd F(2x2,3x3) (wino_kernels.h): 16 weight points, not 9 taps
    Wino43,      // fp32 Winograd F(4x4,3x3) (wino43_kernel.h)
    DeconvDma,   // transposed conv, LDS-DMA staged (deconv_kernel.h): fp32 and bf16
    Bf16Dma,     // bf16 3x3 conv, LDS-DMA staged (conv_bf16_dma.h)
    Bf16Stream,  // ... with a producer wave and the weights in registers: 32 output channels, stream_nch chunks
    Bf16First2,  // ... with conv1_1 (first2_cin input channels) folded into conv1_2's launch
};

struct KernelVariant {
    int TW, MTB, WM, WN, BN, CK;
    bool deconv;
    Family family;
    int TH, lds_bytes;
    int blocks_per_cu;  // resident workgroups per CU (registers and LDS permitting)
    void (*launch)(const ConvArgs&, dim3 grid, hipStream_t s);
    hipError_t (*prepare)();
    bool tail_only = false;  // quarter-size tiles: never a layer's main variant
    bool bf16 = false;       // CB16 bf16 activations (first-layer kernels: bf16 OUTPUT)
    int parts = 1;           // 2: split mode, every map is a hi + lo pair of bf16 maps
    int first2_cin = 0;      // Bf16First2: conv1_1's input channels, 6 / 4
    int stream_nch = 0;      // Bf16Stream: exactly this many 16-channel input chunks
};

// What the conv path reads from the environment, once per process (conv.hip).  The forms behind the switches are
// the references of the tests (each in a child process, held to the default's bars) or documented opt-ins.
struct ConvSwitches {
    int wino;            // DODT_CONV_WINO, dodt_conv_mode(): 2 (default) F(2x2,3x3), 4 F(4x4,3x3), 0 the direct kernels
    bool deconv_dma;     // DODT_CONV_DECONV_DMA=0: transposed convs on the register-staged template
    bool bf16_dma;       // DODT_CONV_BF16_DMA=0: bf16 3x3 convs on the register-staged template
    bool bf16_stream;    // DODT_CONV_BF16_STREAM=0: the level-1 bf16 layers on the plain LDS-DMA kernel
    bool bf16_first2;    // DODT_CONV_BF16_FIRST2=0: conv1_1 and conv1_2 as two launches
    bool bf16_xcd;       // DODT_CONV_BF16_XCD=0: one work queue per launch, not one per group of blocks sharing an XCD
    bool f32_xcd;        // DODT_CONV_F32_XCD=0: the same for the fp32 F(2x2) and transposed-conv kernels
    int debug;           // DODT_CONV_DEBUG: ConvArgs::debug, the kernels' diagnostic bits
    const char* stamp_layer;  // DODT_CONV_STAMP_LAYER=<name>: in-kernel step stamps of that layer's launch
    bool debug_plan;     // DODT_DEBUG_PLAN: print the plan and the skip tables' counts
};
const ConvSwitches& conv_switches();

inline KernelVariant tail_only(KernelVariant v) {
    v.tail_only = true;
    return v;
}

template <int TW, int MTB, int WM, int WN, int BN, bool DECONV, bool BF16 = false, int PARTS = 1>
struct Inst {
    using Cfg = ConvCfg<TW, MTB, WM, WN, BN, DECONV, PARTS>;
    static_assert(Cfg::kLdsBytes <= 160 * 1024, "variant does not fit the LDS");
    static void launch(const ConvArgs& a, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL((conv3x3_mfma_kernel<TW, MTB, WM, WN, BN, DECONV, BF16, PARTS>), grid,
                           dim3(256), Cfg::kLdsBytes, s, a);
    }
    static hipError_t prepare() {
        return hipFuncSetAttribute(
            reinterpret_cast<const void*>(&conv3x3_mfma_kernel<TW, MTB, WM, WN, BN, DECONV, BF16, PARTS>),
            hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLdsBytes);
    }
    static KernelVariant variant() {
        int per_cu = Cfg::kMinWaves;  // one wave of each workgroup per SIMD
        const int by_lds = (160 * 1024) / Cfg::kLdsBytes;
        if (per_cu > by_lds) per_cu = by_lds;
        KernelVariant v{TW, MTB, WM, WN, BN, BF16 ? 16 : kCK, DECONV, Family::Direct, Cfg::TH,
                        Cfg::kLdsBytes, per_cu, &launch, &prepare};
        v.bf16 = BF16;
        v.parts = PARTS;
        return v;
    }
};

template <int TB, int CB>
struct InstWino {
    using Cfg = WinoCfg<TB, CB>;
    static_assert(Cfg::kLdsBytes <= 160 * 1024, "variant does not fit the LDS");
    static void launch(const ConvArgs& a, dim3 grid, hipStream_t s) {
        // the kernel's diagnostic bits (no epilogue, no copies, stamps) exist in an instantiation of their own
        if (conv_switches().debug || conv_switches().stamp_layer)
            hipLaunchKernelGGL((wino3x3_f32_kernel<TB, CB, true>), grid, dim3(256), Cfg::kLdsBytes, s, a);
        else
            hipLaunchKernelGGL((wino3x3_f32_kernel<TB, CB>), grid, dim3(256), Cfg::kLdsBytes, s, a);
    }
    static hipError_t prepare() {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&wino3x3_f32_kernel<TB, CB, true>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLdsBytes);
        if (e != hipSuccess) return e;
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&wino3x3_f32_kernel<TB, CB>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLdsBytes);
    }
    static KernelVariant variant() {
        // TW, MTB (unused), WM, WN, BN, CK, deconv, family, TH, lds, blocks_per_cu
        return KernelVariant{Cfg::TW, 0, 4, 1, Cfg::BN, kCK, false, Family::Wino22, Cfg::TH, Cfg::kLdsBytes,
                             2, &launch, &prepare};
    }
};

struct InstWino43 {
    using Cfg = Wino43Cfg;
    static_assert(Cfg::kLdsBytes <= 160 * 1024, "variant does not fit the LDS");
    static void launch(const ConvArgs& a, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL(wino43_f32_kernel<0>, grid, dim3(256), Cfg::kLdsBytes, s, a);
    }
    static hipError_t prepare() {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&wino43_f32_kernel<0>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLdsBytes);
    }
    static KernelVariant variant() {
        return KernelVariant{Cfg::TW, 0, 4, 1, Cfg::BN, kCK, false, Family::Wino43, Cfg::TH, Cfg::kLdsBytes, 1,
                             &launch, &prepare};
    }
};

template <int CB, bool BF16 = false>
struct InstDeconvDma {
    using Cfg = DeconvCfg<CB>;
    static void launch(const ConvArgs& a, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL((deconv3x3_dma_kernel<CB, BF16>), grid, dim3(256), Cfg::kLdsBytes, s, a);
    }
    static hipError_t prepare() {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&deconv3x3_dma_kernel<CB, BF16>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLdsBytes);
    }
    static KernelVariant variant() {
        KernelVariant v{Cfg::TW, 0, 4, 1, Cfg::BN, BF16 ? 16 : kCK, true, Family::DeconvDma, Cfg::TH, Cfg::kLdsBytes, 2,
                        &launch, &prepare};
        v.bf16 = BF16;
        return v;
    }
};

template <int MT, int NT, int S>
struct InstBf16Dma {
    using Cfg = Bf16DmaCfg<MT, NT, S>;
    static_assert(Cfg::kLdsBytes <= 160 * 1024, "variant does not fit the LDS");
    static void launch(const ConvArgs& a, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL((conv3x3_bf16_dma_kernel<MT, NT, S>), grid, dim3(256), Cfg::kLdsBytes, s, a);
    }
    static hipError_t prepare() {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_bf16_dma_kernel<MT, NT, S>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLdsBytes);
    }
    static KernelVariant variant() {
        int per_cu = (160 * 1024) / Cfg::kLdsBytes;
        constexpr int kMax = S == 2 ? (MT == 2 ? 3 : 2) : 1;      // the kernel's launch bounds
        if (per_cu > kMax) per_cu = kMax;
        KernelVariant v{Cfg::TW, 4 * MT, 4, 1, Cfg::BN, 16, false, Family::Bf16Dma, Cfg::TH, Cfg::kLdsBytes,
                        per_cu, &launch, &prepare};
        v.bf16 = true;
        return v;
    }
};

template <int MT, int NCH, int S>
struct InstBf16Stream {
    using Cfg = Bf16StreamCfg<MT, NCH, S>;
    static_assert(2 * Cfg::kLdsBytes <= 160 * 1024, "two workgroups per CU");
    static void launch(const ConvArgs& a, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL((conv3x3_bf16_stream_kernel<MT, NCH, S>), grid, dim3(256), Cfg::kLdsBytes, s, a);
    }
    static hipError_t prepare() {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_bf16_stream_kernel<MT, NCH, S>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLdsBytes);
    }
    static KernelVariant variant() {
        KernelVariant v{Cfg::TW, Cfg::TH, 3, 1, Cfg::BN, 16, false, Family::Bf16Stream, Cfg::TH, Cfg::kLdsBytes, 2,
                        &launch, &prepare};
        v.bf16 = true;
        v.stream_nch = NCH;
        return v;
    }
};

template <int CIN0, int S>
struct InstBf16First2 {
    using Cfg = Bf16First2Cfg<CIN0, S>;
    static_assert(2 * Cfg::kLdsBytes <= 160 * 1024, "two workgroups per CU");
    static void launch(const ConvArgs& a, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL((conv3x3_bf16_first2_kernel<CIN0, S>), grid, dim3(256), Cfg::kLdsBytes, s, a);
    }
    static hipError_t prepare() {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_bf16_first2_kernel<CIN0, S>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLdsBytes);
    }
    static KernelVariant variant() {
        KernelVariant v{Cfg::TW, Cfg::TH, 3, 1, Cfg::BN, 16, false, Family::Bf16First2, Cfg::TH, Cfg::kLdsBytes, 2,
                        &launch, &prepare};
        v.bf16 = true;
        v.first2_cin = CIN0;
        return v;
    }
};

template <int TW, int MTB, int CK, bool OUT16 = false, bool SPLIT = false>
struct InstSmall {
    using Cfg = SmallCfg<TW, MTB, CK>;
    static void launch(const ConvArgs& a, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL((conv3x3_small_cin_kernel<TW, MTB, CK, OUT16, SPLIT>), grid, dim3(256),
                           Cfg::kLdsBytes, s, a);
    }
    static hipError_t prepare() {
        return hipFuncSetAttribute(
            reinterpret_cast<const void*>(&conv3x3_small_cin_kernel<TW, MTB, CK, OUT16, SPLIT>),
            hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLdsBytes);
    }
    static KernelVariant variant() {
        // (blocks_per_cu as dodt_conv_variant_info has always reported it; launch_grid: three by the kernel's registers)
        KernelVariant v{TW, MTB, 4, 1, 32, CK, false, Family::SmallCin, Cfg::TH, Cfg::kLdsBytes, 4, &launch,
                        &prepare};
        v.bf16 = OUT16;
        v.parts = SPLIT ? 2 : 1;
        return v;
    }
};

// conv_bf16.hip, conv_split.hip
std::vector<KernelVariant> bf16_variants();
std::vector<KernelVariant> split_variants();

}  // namespace dodt
