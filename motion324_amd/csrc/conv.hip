// The 3 x 3 convolution and the 2 x 2 max-pool behind the perceptual evaluation (LPIPS on a VGG16 trunk, csrc/perceptual.hip) and
// the foreground matting (U2-Net, csrc/matting.hip): one kernel template and one host path for m324_conv3x3 and m324_conv3x3_ex,
// one pool kernel for m324_maxpool2x2 and m324_maxpool2x2_ceil.  The contract of every entry point is in include/m324.h; what is
// here is how.
//
// The convolution is an implicit GEMM on the fp32-input MFMA (v_mfma_f32_32x32x2_f32): M = the pixels of all images, N = Cout,
// K = 9 Cin in (tap, channel) order.  The taps lie `dilation` pixels apart, and the K axis runs over the channels of TWO tensors (a
// piece of four channels comes from `a` when c < Ca and from `b` otherwise; Ca % 4 = 0, so no piece straddles them and the
// concatenation never exists in memory); m324_conv3x3 is the call with b = NULL, res = NULL and dilation 1.  A workgroup of four
// waves owns a tile of 128 pixels by BN = 128, 64 or 32 output channels.  A K step is 16 values: four 16-byte pieces per pixel,
// each piece four channels of ONE tap (Cin % 4 = 0), fetched from the NHWC activation at (y + dy, x + dx) or replaced by zeros
// when that lies outside the image, the pixel is past M or k is past 9 Cin.  The pieces go to LDS transposed ([k][pixel]) so that
// the 32 lanes of an A operand read 32 neighbouring words; the weights are stored [k][Cout] already and go in as they are.
// Two LDS stages: the loads of step s + 1 are issued before the MFMAs of step s and stored behind them, one barrier per step.
// No LDS-DMA and no cross-lane arithmetic.
//
// The sum over k has two levels: the MFMA's fma chain runs over M324_CONV_RUN = 144 consecutive k (nine K steps) from 0.0f, then
// the accumulators are added to a second set and cleared.  One chain over all 4608 k of a 512-channel layer has a rounding error
// that grows with the running sum: measured against fp64, the deep taps of the metric came out 3 to 10 times further off than a
// blocked CPU sum and outside the tests' gate; with runs of 144 they are as close as that.  The cost is 64 v_add_f32 per wave
// every 288 MFMAs.  Every output is the same fixed sequence of operations whatever its pixel's place in a tile, in the grid or in
// the batch, then + bias, max(., 0) and + res.
//
// What varies with the layer is the tile only.  BN = 128 and 64 split the tile over 2 x 2 waves, every wave 64 x BN/2 of it as
// 2 x BN/64 accumulator tiles; BN = 32 stacks the four waves along the pixels, one 32 x 32 accumulator each, so that a 16- or
// 32-channel layer wastes at most the columns past Cout of ONE 32-wide tile (the fp32 MFMA whose chain the contract states is 32
// wide).  A 256 x 64 tile of four 64 x 64 waves, which has the MFMA-to-LDS-read ratio of the 128-wide tile, was measured for the
// 64-channel layers and lost 4 to 10 % against 128 x 64 (184 VGPRs and 45 KB of LDS: fewer waves per CU); profiles/matting.md has
// the numbers.  An output's bits do not depend on the tile: every tile runs the same chain for it.  The two entry points differ in
// the rule that picks the tile (below, at the entry points) and in what they accept, in nothing else.
//
// m324_conv3x3_s2 (ISNet's stem) is the same kernel with one more compile-time parameter, STRIDE = 2: the pixels of M, of the tiles
// and of the epilogue are those of the OUTPUT [images, Ho, Wo], and the prologue turns each into the source pixel (2 y, 2 x) it is
// centred on; from there the fetch is the one above, bounds against (H, W) included.  So an output runs the chain that the stride-1
// kernel runs for the source pixel (2 y, 2 x), and has its bits.  STRIDE = 1 compiles to the code it was: the gather is an `if
// constexpr` in the prologue.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int BM = 128;
constexpr int BK = M324_CONV_KPAD;
constexpr int RUN_STEPS = M324_CONV_RUN / BK;
constexpr int FILL_WORKGROUPS = 512;    // below this many 128-wide tiles the chip is not full and m324_conv3x3_ex takes the narrower tile

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// WN waves along the channels, 4 / WN along the pixels.  PLAIN is m324_conv3x3's call (one source, dilation 1, no residual) with
// b, Cb, dil and res folded away at compile time: the general kernel was measured 1.3 % slower on LPIPS without it
// (profiles/conv_unified.md).  The operations on the data and their order are the same.
template <int BN, int WN, bool PLAIN, int STRIDE>
__global__ __launch_bounds__(THREADS) void conv3x3_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ wp,
                                                          const float* __restrict__ bias, const float* __restrict__ res, float* __restrict__ out,
                                                          long M, int H, int W, int Ca, int Cb, int Cout, int K, int n_tiles, int dil, int relu) {
    constexpr int NP = BM / 64;                     // pixels this thread fetches per step
    constexpr int LDA = BM + 4;                     // 4 * LDA = 16 mod 64: the four pieces of 16 pixels land in 64 different banks
    constexpr int TM = BM / (32 * (4 / WN));        // 32-row accumulator tiles per wave
    constexpr int TN = BN / (32 * WN);              // 32-column accumulator tiles per wave
    constexpr int LDB = BN % 64 == 0 ? BN + 32 : BN;        // LDB = 32 mod 64: the two k rows of a B operand read disjoint banks
    constexpr int BPIECES = BK * BN / 4;            // 16-byte pieces of the weight tile
    constexpr int BQ = (BPIECES + THREADS - 1) / THREADS;
    __shared__ float As[2][BK * LDA];
    __shared__ float Bs[2][BK * LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long m0 = (long)(blockIdx.x / n_tiles) * BM;
    const int n0 = (blockIdx.x % n_tiles) * BN;
    const int C = PLAIN ? Ca : Ca + Cb;

    // the NP pixels this thread fetches, and the piece (four channels) of the step it fetches for all of them
    const int kq = tid & 3;
    long pix[NP];
    int px[NP], py[NP];
    bool pv[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const long p = m0 + (tid >> 2) + 64 * i;
        pv[i] = p < M;
        pix[i] = pv[i] ? p : 0;
        if constexpr (STRIDE == 1) {
            px[i] = (int)(pix[i] % W);
            py[i] = (int)((pix[i] / W) % H);
        } else {                                    // p counts output pixels; pix, px, py become the source pixel it is centred on
            const int Ho = (H - 1) / STRIDE + 1, Wo = (W - 1) / STRIDE + 1;
            px[i] = (int)(pix[i] % Wo) * STRIDE;
            py[i] = (int)((pix[i] / Wo) % Ho) * STRIDE;
            pix[i] = ((pix[i] / ((long)Wo * Ho)) * H + py[i]) * W + px[i];
        }
    }
    int bk[BQ], bn[BQ];
    bool bv[BQ];
#pragma unroll
    for (int i = 0; i < BQ; ++i) {
        const int idx = tid + THREADS * i;
        bv[i] = idx < BPIECES;
        bk[i] = bv[i] ? idx / (BN / 4) : 0;
        bn[i] = bv[i] ? (idx % (BN / 4)) * 4 : 0;
        bv[i] = bv[i] && n0 + bn[i] < Cout;
    }

    float4 ra[NP], rb[BQ];
    auto fetch = [&](int k0) {
        const int k = k0 + kq * 4;
        const int tap = k / C, c = k - tap * C;
        const int d = PLAIN ? 1 : dil;
        const int dy = (tap / 3 - 1) * d, dx = (tap - (tap / 3) * 3 - 1) * d;
        const bool first = PLAIN || c < Ca;
        const float* src = first ? a : b;
        const int cs = first ? Ca : Cb, cc = first ? c : c - Ca;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const bool ok = pv[i] && k < K && (unsigned)(py[i] + dy) < (unsigned)H && (unsigned)(px[i] + dx) < (unsigned)W;
            ra[i] = ok ? *reinterpret_cast<const float4*>(src + (pix[i] + (long)dy * W + dx) * cs + cc) : zero4();
        }
#pragma unroll
        for (int i = 0; i < BQ; ++i)
            rb[i] = bv[i] ? *reinterpret_cast<const float4*>(wp + (long)(k0 + bk[i]) * Cout + n0 + bn[i]) : zero4();
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            float* s = &As[buf][(kq * 4) * LDA + (tid >> 2) + 64 * i];
            s[0] = ra[i].x; s[LDA] = ra[i].y; s[2 * LDA] = ra[i].z; s[3 * LDA] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < BQ; ++i)
            if (tid + THREADS * i < BPIECES) *reinterpret_cast<float4*>(&Bs[buf][bk[i] * LDB + bn[i]]) = rb[i];
    };

    f32x16 acc[TM][TN], tot[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = tot[i][j][r] = 0.f;

    const int wm = (wave / WN) * (32 * TM), wn = (wave % WN) * (32 * TN);
    const int l31 = lane & 31, lh = lane >> 5;
    const int steps = (K + BK - 1) / BK;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int buf = s & 1;
        if (s + 1 < steps) fetch((s + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const int k = 2 * kk + lh;              // lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31]
            float av[TM], bw[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = As[buf][k * LDA + wm + 32 * i + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) bw[j] = Bs[buf][k * LDB + wn + 32 * j + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bw[j], acc[i][j], 0, 0, 0);
        }
        if ((s + 1) % RUN_STEPS == 0) {             // a run of M324_CONV_RUN products ends: second level of the sum
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        tot[i][j][r] += acc[i][j][r];
                        acc[i][j][r] = 0.f;
                    }
        }
        if (s + 1 < steps) stage(buf ^ 1);          // last read in step s - 1, behind that step's barrier
        __syncthreads();
    }

    // C/D of the 32 x 32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn + 32 * j + l31;
        if (n >= Cout) continue;
        const float bv0 = bias[n];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long p = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (p < M) {
                    float v = (tot[i][j][r] + acc[i][j][r]) + bv0;
                    if (relu) v = v > 0.f ? v : 0.f;
                    if (!PLAIN && res) v = v + res[p * Cout + n];
                    out[p * Cout + n] = v;
                }
            }
    }
}

__device__ __forceinline__ float4 max4(float4 a, float4 b) {
    return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

__global__ __launch_bounds__(THREADS) void maxpool2x2_kernel(const float4* __restrict__ in, float4* __restrict__ out, long total, int H, int W,
                                                             int Ho, int Wo, int C4) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    long r = i / C4;
    const int x = (int)(r % Wo);
    r /= Wo;
    const int y = (int)(r % Ho);
    const long img = r / Ho;
    const bool right = 2 * x + 1 < W, below = 2 * y + 1 < H;      // the window is cut at the edge
    const float4* s = in + ((img * H + 2 * y) * W + 2 * x) * C4 + c;
    float4 v = s[0];
    if (right) v = max4(v, s[C4]);
    if (below) v = max4(v, s[(long)W * C4]);
    if (right && below) v = max4(v, s[(long)W * C4 + C4]);
    out[i] = v;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// m324_conv3x3_ex's tile width from Cout and the pixel count M: the widest one that divides Cout while it still fills the chip
int tile_of(long M, int Cout) {
    if (Cout % 128 == 0 && (M + BM - 1) / BM * (Cout / 128) >= FILL_WORKGROUPS) return 128;
    return Cout > 32 ? 64 : 32;
}

// The contract the convolutions share, then the launch with the tile `width` (128, 64 or 32) that the caller `name` chose;
// `plain` (m324_conv3x3: b, res null, dilation 1, width 128 or 64) takes the kernels with those folded away; `stride` 2
// (m324_conv3x3_s2, never plain) counts M, the tiles and the grid in output pixels
int conv3x3(const char* name, int width, bool plain, int stride, const float* a, int Ca, const float* b, int Cb, const float* wp, const float* bias,
            const float* res, float* out, int images, int H, int W, int Cout, int dilation, int relu, void* stream) {
    M324_REQUIRE(a && wp && bias && out, "%s: null a, wp, bias or out", name);
    M324_REQUIRE(images >= 1 && H >= 1 && W >= 1, "%s: images, H and W must be at least 1, got %d, %d, %d", name, images, H, W);
    M324_REQUIRE(Ca >= 4 && Ca % 4 == 0, "%s: Ca must be a positive multiple of 4, got %d", name, Ca);
    M324_REQUIRE((b == nullptr && Cb == 0) || (b != nullptr && Cb >= 4 && Cb % 4 == 0),
                 "%s: Cb must be 0 with b null, or a positive multiple of 4 with b given, got %d", name, Cb);
    M324_REQUIRE(Cout >= 4 && Cout % 4 == 0, "%s: Cout must be a positive multiple of 4, got %d", name, Cout);
    M324_REQUIRE(Ca <= M324_CONV_MAX_CHANNELS && Cb <= M324_CONV_MAX_CHANNELS && Ca + Cb <= M324_CONV_MAX_CHANNELS && Cout <= M324_CONV_MAX_CHANNELS,
                 "%s: at most %d channels (Ca + Cb, and Cout), got Ca %d, Cb %d, Cout %d", name, M324_CONV_MAX_CHANNELS, Ca, Cb, Cout);
    M324_REQUIRE((long)images * H * W <= 0x7fffffffL && (long)H * W <= 0x7fffffffL, "%s: images * H * W must stay below 2^31, got %ld", name,
                 (long)images * H * W);
    const long M = (long)images * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    M324_REQUIRE(dilation >= 1 && dilation <= M324_CONV_MAX_DILATION, "%s: dilation must be in 1..%d, got %d", name, M324_CONV_MAX_DILATION, dilation);
    M324_REQUIRE(aligned16(a) && aligned16(b) && aligned16(wp) && aligned16(out), "%s: a, b, wp and out must be 16-byte aligned", name);
    M324_REQUIRE(((uintptr_t)bias & 3) == 0 && ((uintptr_t)res & 3) == 0, "%s: bias and res must be 4-byte aligned", name);
    M324_REQUIRE(relu == 0 || relu == 1, "%s: relu is 0 or 1, got %d", name, relu);
    const int K = 9 * (Ca + Cb);
    const int n_tiles = (Cout + width - 1) / width;
    const dim3 grid((unsigned)((M + BM - 1) / BM * n_tiles));
    hipStream_t st = (hipStream_t)stream;
#define M324_CONV_LAUNCH(BN_, WN_, PLAIN_, STRIDE_)                                                                                            \
    hipLaunchKernelGGL((conv3x3_kernel<BN_, WN_, PLAIN_, STRIDE_>), grid, dim3(THREADS), 0, st, a, b, wp, bias, res, out, M, H, W, Ca, Cb, Cout, K, \
                       n_tiles, dilation, relu)
    if (stride == 2 && width == 128)
        M324_CONV_LAUNCH(128, 2, false, 2);
    else if (stride == 2 && width == 64)
        M324_CONV_LAUNCH(64, 2, false, 2);
    else if (stride == 2)
        M324_CONV_LAUNCH(32, 1, false, 2);
    else if (plain && width == 128)
        M324_CONV_LAUNCH(128, 2, true, 1);
    else if (plain)
        M324_CONV_LAUNCH(64, 2, true, 1);
    else if (width == 128)
        M324_CONV_LAUNCH(128, 2, false, 1);
    else if (width == 64)
        M324_CONV_LAUNCH(64, 2, false, 1);
    else
        M324_CONV_LAUNCH(32, 1, false, 1);
#undef M324_CONV_LAUNCH
    M324_CHECK_LAUNCH(name);
    return M324_OK;
}

// The contract both pools share, then the launch; an even H and W is the case where no window is cut
int maxpool2x2(const char* name, const float* in, float* out, int images, int H, int W, int C, void* stream) {
    M324_REQUIRE(in && out, "%s: null in or out", name);
    M324_REQUIRE(images >= 1 && H >= 1 && W >= 1, "%s: images, H and W must be at least 1, got %d, %d, %d", name, images, H, W);
    M324_REQUIRE(C >= 4 && C % 4 == 0 && C <= M324_CONV_MAX_CHANNELS, "%s: C must be a multiple of 4 in 4..%d, got %d", name, M324_CONV_MAX_CHANNELS, C);
    M324_REQUIRE((long)images * H * W <= 0x7fffffffL, "%s: images * H * W must stay below 2^31", name);
    M324_REQUIRE(aligned16(in) && aligned16(out), "%s: in and out must be 16-byte aligned", name);
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const long total = (long)images * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, (const float4*)in,
                       (float4*)out, total, H, W, Ho, Wo, C / 4);
    M324_CHECK_LAUNCH(name);
    return M324_OK;
}

}  // namespace

// m324_conv3x3's own tile rule: 128 wide whenever that divides Cout, whatever the pixel count, and never the 32-wide tile
extern "C" int m324_conv3x3(const float* in, const float* wp, const float* bias, float* out, int images, int H, int W, int Cin, int Cout,
                            int relu, void* stream) {
    M324_REQUIRE(Cout >= 32 && Cout % 32 == 0, "m324_conv3x3: Cout must be a positive multiple of 32, got %d", Cout);
    return conv3x3("m324_conv3x3", Cout % 128 == 0 ? 128 : 64, true, 1, in, Cin, nullptr, 0, wp, bias, nullptr, out, images, H, W, Cout, 1, relu, stream);
}

extern "C" int m324_conv3x3_ex(const float* a, int Ca, const float* b, int Cb, const float* wp, const float* bias, const float* res, float* out,
                               int images, int H, int W, int Cout, int dilation, int relu, void* stream) {
    return conv3x3("m324_conv3x3_ex", tile_of((long)images * H * W, Cout), false, 1, a, Ca, b, Cb, wp, bias, res, out, images, H, W, Cout, dilation, relu, stream);
}

// stride 2, zero padding 1: one source, no residual; the tile rule is m324_conv3x3_ex's on the OUTPUT pixel count
extern "C" int m324_conv3x3_s2(const float* in, const float* wp, const float* bias, float* out, int images, int H, int W, int Cin, int Cout,
                               int relu, void* stream) {
    M324_REQUIRE(images >= 1 && H >= 1 && W >= 1, "m324_conv3x3_s2: images, H and W must be at least 1, got %d, %d, %d", images, H, W);
    const long Mo = (long)images * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    return conv3x3("m324_conv3x3_s2", tile_of(Mo, Cout), false, 2, in, Cin, nullptr, 0, wp, bias, nullptr, out, images, H, W, Cout, 1, relu, stream);
}

extern "C" int m324_conv3x3_ex_tile(int images, int H, int W, int Cout) {
    if (images < 1 || H < 1 || W < 1 || Cout < 4 || Cout % 4) return M324_ERR_INVALID;
    return tile_of((long)images * H * W, Cout);
}

extern "C" int m324_maxpool2x2(const float* in, float* out, int images, int H, int W, int C, void* stream) {
    M324_REQUIRE(images >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "m324_maxpool2x2: images >= 1 and even H, W >= 2, got %d, %d, %d",
                 images, H, W);
    return maxpool2x2("m324_maxpool2x2", in, out, images, H, W, C, stream);
}

extern "C" int m324_maxpool2x2_ceil(const float* in, float* out, int images, int H, int W, int C, void* stream) {
    return maxpool2x2("m324_maxpool2x2_ceil", in, out, images, H, W, C, stream);
}
