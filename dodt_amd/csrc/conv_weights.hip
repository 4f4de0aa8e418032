// Weight blocking of the VGG-pyramid extractor (dodt_extractor_set_layer): host functions from a layer's TF-layout
// weights to the array a kernel variant reads.  Channels a layer pads (cin < l.Cin) stay zero.
#include <array>

#include "extractor.h"

namespace dodt {

// transposed conv, TF layout (kh, kw, Cout, Cin): blocked [n-tile][chunk][tap][g = c / 2][t]
// [channel block][c & 1]: a lane (t, g) reads 16 bytes = its channel pair for both blocks
// (bf16: the same bytes hold 16 channels per chunk, [g = c / 4] ... [c & 3] as bf16)
std::vector<float> block_deconv_dma(const WeightTile& v, const Layer& l, const float* w, int cin, int cout) {
    const int nchunks = l.Cin / v.CK;
    const int ncb = v.BN / 16;
    const size_t chunk_floats = (size_t)(9 * 8 * v.BN + 255) / 256 * 256;     // whole 1 KB pieces
    std::vector<float> u((size_t)(l.Cout / v.BN) * nchunks * chunk_floats, 0.0f);
    uint16_t* u16 = reinterpret_cast<uint16_t*>(u.data());
    for (int tap = 0; tap < 9; ++tap)
        for (int ci = 0; ci < cin; ++ci)
            for (int co = 0; co < cout; ++co) {
                const float val = w[((size_t)tap * cout + co) * cin + ci];
                const int nt = co / v.BN, n = co % v.BN, cb = n / 16, t = n % 16;
                if (v.bf16) {
                    const int ch = ci / 16, c = ci % 16;
                    u16[(((size_t)nt * nchunks + ch) * chunk_floats) * 2 +
                        ((((size_t)tap * 4 + c / 4) * 16 + t) * ncb + cb) * 4 + (c & 3)] = float_to_bf16(val);
                } else {
                    const int ch = ci / 8, c = ci % 8;
                    u[((size_t)nt * nchunks + ch) * chunk_floats +
                      ((((size_t)tap * 4 + c / 2) * 16 + t) * ncb + cb) * 2 + (c & 1)] = val;
                }
            }
    return u;
}

// F(4x4,3x3) filter transform U = G g G^T (6x6 points; float64 on the host, rounded once),
// blocked [n-tile][chunk][xi / 2][g = c / 2][cb][t][xi & 1][c & 1]: a lane (t, g) of channel
// block cb reads 16 bytes = its channel pair for two points
std::vector<float> block_wino43(const WeightTile& v, const Layer& l, const float* w, int cin, int cout) {
    const int nchunks = l.Cin / v.CK;
    // points 0, +-2/3, +-3/2, infinity (wino43_kernel.h): G[j][k] = p_j^k / prod_{l != j} (p_j - p_l)
    static const std::array<std::array<double, 3>, 6> G = [] {
        const double p[5] = {0.0, 2.0 / 3.0, -2.0 / 3.0, 1.5, -1.5};
        std::array<std::array<double, 3>, 6> g{};
        for (int j = 0; j < 5; ++j) {
            double n = 1.0;
            for (int l = 0; l < 5; ++l)
                if (l != j) n *= p[j] - p[l];
            g[j] = {1.0 / n, p[j] / n, p[j] * p[j] / n};
        }
        g[5] = {0.0, 0.0, 1.0};
        return g;
    }();
    std::vector<float> u((size_t)36 * l.Cin * l.Cout, 0.0f);
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co) {
            double gk[3][3], tmp[6][3];
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx)
                    gk[ky][kx] = w[((size_t)(ky * 3 + kx) * cin + ci) * cout + co];
            for (int i = 0; i < 6; ++i)
                for (int kx = 0; kx < 3; ++kx)
                    tmp[i][kx] = G[i][0] * gk[0][kx] + G[i][1] * gk[1][kx] + G[i][2] * gk[2][kx];
            const int nt = co / v.BN, n = co % v.BN, ch = ci / 8, c = ci % 8;
            const int cb = n / 16, t = n % 16;
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) {
                    const double val = tmp[i][0] * G[j][0] + tmp[i][1] * G[j][1] + tmp[i][2] * G[j][2];
                    const int xi = i * 6 + j;
                    u[(((((((size_t)nt * nchunks + ch) * 18 + xi / 2) * 4 + c / 2) * 2 + cb) * 16 + t) * 2 +
                       (xi & 1)) * 2 + (c & 1)] = (float)val;
                }
        }
    return u;
}

// Winograd F(2x2,3x3) filter transform U = G g G^T (float64 on the host, rounded once to fp32),
// G = [[1,0,0],[1/2,1/2,1/2],[1/2,-1/2,1/2],[0,0,1]]; blocked like the direct kernel's
// weights with the 16 points in place of the 9 taps: [n-tile][chunk][xi][h][n][4]
std::vector<float> block_wino22(const WeightTile& v, const Layer& l, const float* w, int cin, int cout) {
    const int nchunks = l.Cin / v.CK;
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<float> u((size_t)16 * l.Cin * l.Cout, 0.0f);
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co) {
            double gk[3][3], tmp[4][3];
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx)
                    gk[ky][kx] = w[((size_t)(ky * 3 + kx) * cin + ci) * cout + co];
            for (int i = 0; i < 4; ++i)
                for (int kx = 0; kx < 3; ++kx)
                    tmp[i][kx] = G[i][0] * gk[0][kx] + G[i][1] * gk[1][kx] + G[i][2] * gk[2][kx];
            // [n-tile][chunk][xi][g = c/2][cb pair][t][cb & 1][k = c%2]: a lane (t, g) of the
            // kernel reads 16 bytes = its (2g, 2g+1) channel pair for two 16-channel blocks
            const int nt = co / v.BN, n = co % v.BN, ch = ci / 8, c = ci % 8;
            const int cb = n / 16, t = n % 16, cbp = v.BN / 32;
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    const double val = tmp[i][0] * G[j][0] + tmp[i][1] * G[j][1] + tmp[i][2] * G[j][2];
                    u[((((((size_t)nt * nchunks + ch) * 16 + (i * 4 + j)) * 4 + c / 2) * cbp + cb / 2) * 16 + t) * 4 +
                      (cb % 2) * 2 + c % 2] = (float)val;
                }
        }
    return u;
}

// the direct kernels.  fp32 kernels: floats; bf16 MFMA kernels: bf16 pairs packed in the same array (half of it)
std::vector<float> block_direct(const WeightTile& v, const Layer& l, const float* w, int cin, int cout) {
    const int nchunks = l.Cin / v.CK;
    std::vector<float> blocked((size_t)9 * l.Cin * l.Cout, 0.0f);
    uint16_t* blocked16 = reinterpret_cast<uint16_t*>(blocked.data());
    const bool w16 = v.bf16 && !v.small_cin;
    for (int tap = 0; tap < 9; ++tap)
        for (int ci = 0; ci < cin; ++ci)
            for (int co = 0; co < cout; ++co) {
                const float val = l.deconv ? w[((size_t)tap * cout + co) * cin + ci]
                                           : w[((size_t)tap * cin + ci) * cout + co];
                int n = co % v.BN;
                if (v.bf16) {
                    // MFMA row that delivers channel co (conv_kernels.h group_channel<PERM>):
                    // channel 16a + 8lh + 4b + k  <-  row 8(2a + b) + 4lh + k
                    const int c32 = co % 32, a2 = c32 >> 4, lh = (c32 >> 3) & 1, b2 = (c32 >> 2) & 1;
                    n = (n / 32) * 32 + 8 * (2 * a2 + b2) + 4 * lh + (c32 & 3);
                }
                const int nt = co / v.BN, ch = ci / v.CK, c = ci % v.CK;
                if (v.small_cin) {   // [tap][c][n]
                    blocked[((size_t)tap * v.CK + c) * v.BN + n] = val;
                } else if (!w16) {   // [n_tile][chunk][tap][h = c/4][n][s = c%4]
                    blocked[(((((size_t)nt * nchunks + ch) * 9 + tap) * 2 + c / 4) * v.BN + n) * 4 +
                            c % 4] = val;
                } else {   // [n_tile][chunk16][part][tap][h = c/8][n][j = c%8] bf16
                    const uint16_t hi = float_to_bf16(val);
                    const size_t base = ((size_t)nt * nchunks + ch) * v.parts;
                    const size_t in = ((size_t)(tap * 2 + c / 8) * v.BN + n) * 8 + c % 8;
                    blocked16[(base + 0) * 9 * 2 * v.BN * 8 + in] = hi;
                    if (v.parts == 2)    // lo = bf16(w - hi): w = hi + lo to 16 mantissa bits
                        blocked16[(base + 1) * 9 * 2 * v.BN * 8 + in] =
                            float_to_bf16(val - bf16_to_float(hi));
                }
            }
    return blocked;
}

// conv1_1 for conv3x3_bf16_first2_kernel: A fragments [K = 16 step][hi, lo][lane half][32 MFMA rows][8 bf16];
// a lane half's eight K slots are one tap's six channels + two zeros (Cin 6: taps 2 s + lh) or two taps' four
// channels (Cin 4: taps 4 s + 2 lh, + 1); w = hi + lo to 16 mantissa bits
std::vector<uint16_t> pack_first2(const Layer& l, const float* w, int cin, int cout) {
    const int steps = l.Cin == 6 ? 5 : 3;
    std::vector<uint16_t> frag((size_t)steps * 2 * 2 * 32 * 8, 0);
    for (int st = 0; st < steps; ++st)
        for (int lh = 0; lh < 2; ++lh)
            for (int row = 0; row < 32; ++row) {
                // channel of MFMA row 8 (2 a + b) + 4 lh' + k: 16 a + 8 lh' + 4 b + k (group_channel<true>)
                const int g = row >> 3, lho = (row >> 2) & 1, co = 16 * (g >> 1) + 8 * lho + 4 * (g & 1) + (row & 3);
                for (int j = 0; j < 8; ++j) {
                    const int tap = l.Cin == 6 ? 2 * st + lh : 4 * st + 2 * lh + (j >> 2);
                    const int ci = l.Cin == 6 ? j : (j & 3);
                    if (tap >= 9 || ci >= cin) continue;
                    const float val = w[((size_t)tap * cin + ci) * cout + co];
                    const uint16_t hi = float_to_bf16(val);
                    const size_t at = ((((size_t)st * 2 + 0) * 2 + lh) * 32 + row) * 8 + j;
                    frag[at] = hi;
                    frag[at + 2 * 32 * 8] = float_to_bf16(val - bf16_to_float(hi));
                }
            }
    return frag;
}

}  // namespace dodt
