// Perceptual evaluation (LPIPS on a VGG16 trunk): the 3 x 3 convolution, the 2 x 2 max-pool, the input scaling and the
// normalise-subtract-square-weigh head.  The contract of every entry point is in include/m324.h; what is here is how.
//
// m324_conv3x3 is an implicit GEMM on the fp32-input MFMA (v_mfma_f32_32x32x2_f32): M = the pixels of all images, N = Cout,
// K = 9 Cin in (tap, channel) order.  A workgroup of four waves owns a 128 x BN tile (BN = 128, or 64 when Cout is no multiple
// of 128), every wave 64 x BN/2 of it as 2 x BN/64 accumulator tiles.  A K step is 16 values: four 16-byte pieces per pixel,
// each piece four channels of ONE tap (Cin % 4 = 0), fetched from the NHWC activation at (y + dy, x + dx) or replaced by zeros
// when that lies outside the image, the pixel is past M or k is past 9 Cin.  The pieces go to LDS transposed ([k][pixel]) so that
// the 32 lanes of an A operand read 32 neighbouring words; the weights are stored [k][Cout] already and go in as they are.
// Two LDS stages: the loads of step s + 1 are issued before the MFMAs of step s and stored behind them, one barrier per step.
// No LDS-DMA and no cross-lane arithmetic.  The sum over k has two levels: the MFMA's fma chain runs over M324_CONV_RUN = 144
// consecutive k (nine K steps) from 0.0f, then the accumulators are added to a second set and cleared.  One chain over all
// 4608 k of a 512-channel layer has a rounding error that grows with the running sum: measured against fp64, the deep taps of
// the metric came out 3 to 10 times further off than a blocked CPU sum and outside the tests' gate; with runs of 144 they are
// as close as that.  The cost is 64 v_add_f32 per wave every 288 MFMAs.  Every output is the same fixed sequence of operations
// whatever its pixel's place in a tile, in the grid or in the batch, then + bias and max(., 0).
#include "common.h"
#include <math.h>

namespace {

constexpr int THREADS = 256;
constexpr int BM = 128;
constexpr int BK = M324_CONV_KPAD;
constexpr int RUN_STEPS = M324_CONV_RUN / BK;
constexpr int LDA = BM + 4;             // 4 * LDA = 16 mod 64: the four pieces of 16 pixels land in 64 different banks

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

template <int BN>
__global__ __launch_bounds__(THREADS) void conv3x3_kernel(const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ bias,
                                                          float* __restrict__ out, long M, int H, int W, int Cin, int Cout, int K, int n_tiles,
                                                          int relu) {
    constexpr int LDB = BN + 32;        // LDB = 32 mod 64: the two k rows of a B operand read disjoint banks
    constexpr int TN = BN / 64;         // 32-column accumulator tiles per wave
    constexpr int BQ = BK * BN / 4 / THREADS;       // 16-byte pieces of the weight tile per thread
    __shared__ float As[2][BK * LDA];
    __shared__ float Bs[2][BK * LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long m0 = (long)(blockIdx.x / n_tiles) * BM;
    const int n0 = (blockIdx.x % n_tiles) * BN;

    // the two pixels this thread fetches, and the piece (four channels) of the step it fetches for both
    const int kq = tid & 3;
    long pix[2];
    int px[2], py[2];
    bool pv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long p = m0 + (tid >> 2) + 64 * i;
        pv[i] = p < M;
        pix[i] = pv[i] ? p : 0;
        px[i] = (int)(pix[i] % W);
        py[i] = (int)((pix[i] / W) % H);
    }
    int bk[BQ], bn[BQ];
#pragma unroll
    for (int i = 0; i < BQ; ++i) {
        const int idx = tid + THREADS * i;
        bk[i] = idx / (BN / 4);
        bn[i] = (idx % (BN / 4)) * 4;
    }

    float4 ra[2], rb[BQ];
    auto fetch = [&](int k0) {
        const int k = k0 + kq * 4;
        const int tap = k / Cin, c = k - tap * Cin;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool ok = pv[i] && k < K && (unsigned)(py[i] + dy) < (unsigned)H && (unsigned)(px[i] + dx) < (unsigned)W;
            ra[i] = ok ? *reinterpret_cast<const float4*>(in + (pix[i] + (long)dy * W + dx) * Cin + c) : zero4();
        }
#pragma unroll
        for (int i = 0; i < BQ; ++i)
            rb[i] = n0 + bn[i] < Cout ? *reinterpret_cast<const float4*>(wp + (long)(k0 + bk[i]) * Cout + n0 + bn[i]) : zero4();
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float* a = &As[buf][(kq * 4) * LDA + (tid >> 2) + 64 * i];
            a[0] = ra[i].x; a[LDA] = ra[i].y; a[2 * LDA] = ra[i].z; a[3 * LDA] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < BQ; ++i) *reinterpret_cast<float4*>(&Bs[buf][bk[i] * LDB + bn[i]]) = rb[i];
    };

    f32x16 acc[2][TN], tot[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = tot[i][j][r] = 0.f;

    const int wm = (wave >> 1) * 64, wn = (wave & 1) * (BN / 2);
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
            float a[2], b[TN];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[buf][k * LDA + wm + 32 * i + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[buf][k * LDB + wn + 32 * j + l31];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if ((s + 1) % RUN_STEPS == 0) {             // a run of M324_CONV_RUN products ends: second level of the sum
#pragma unroll
            for (int i = 0; i < 2; ++i)
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
        const float bv = bias[n];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long p = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (p < M) {
                    float v = (tot[i][j][r] + acc[i][j][r]) + bv;
                    if (relu) v = v > 0.f ? v : 0.f;
                    out[p * Cout + n] = v;
                }
            }
    }
}

__global__ __launch_bounds__(THREADS) void maxpool2x2_kernel(const float4* __restrict__ in, float4* __restrict__ out, long total, int Ho, int Wo, int C4) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    long r = i / C4;
    const int x = (int)(r % Wo);
    r /= Wo;
    const int y = (int)(r % Ho);
    const long img = r / Ho;
    const long row = 2L * Wo * C4;                  // one input row, in float4
    const float4* s = in + ((img * 2 * Ho + 2 * y) * 2 * Wo + 2 * x) * C4 + c;
    const float4 a = s[0], b = s[C4], d = s[row], e = s[row + C4];
    out[i] = make_float4(fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, e.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y)),
                         fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, e.z)), fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, e.w)));
}

// y_c = (x_c - shift_c) / scale_c, x = (v / 255) * 2 - 1 for a byte: as written, nothing fused into an fma
__global__ __launch_bounds__(THREADS) void lpips_prepare_kernel(const void* __restrict__ src, int mode, int normalize, long total, long HW,
                                                                float4* __restrict__ dst) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    float x[3];
    if (mode == M324_LPIPS_U8_NHWC) {
        const unsigned char* s = (const unsigned char*)src + 3 * i;
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = ((float)s[c] / 255.0f) * 2.0f - 1.0f;
    } else {
        const long img = i / HW, p = i - img * HW;
        const float* s = (const float*)src + img * 3 * HW + p;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = s[c * HW];
            x[c] = normalize ? v * 2.0f - 1.0f : v;
        }
    }
    dst[i] = make_float4((x[0] - -0.030f) / 0.458f, (x[1] - -0.088f) / 0.448f, (x[2] - -0.188f) / 0.450f, 0.f);
}

// G lanes share a pixel: lane gl holds channels 4 (gl + q G) .. + 3, q < HEAD_Q.  A butterfly over the G lanes leaves the same
// sum in each of them (a + b = b + a at every level).

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = 1; off < G; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int G, int HEAD_Q>
__global__ __launch_bounds__(THREADS) void lpips_layer_kernel(const float* __restrict__ fa, const float* __restrict__ fb, const float* __restrict__ w,
                                                              long HW, int C, int chunks, float* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int NG = THREADS / G;
    __shared__ float red[NG];
    const int tid = threadIdx.x, gl = tid % G, g = tid / G;
    const long pair = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const long per = (HW + chunks - 1) / chunks;
    const long p0 = chunk * per, p1 = p0 + per < HW ? p0 + per : HW;
    const int C4 = C / 4;
    float4 wv[HEAD_Q];
#pragma unroll
    for (int q = 0; q < HEAD_Q; ++q) wv[q] = gl + q * G < C4 ? reinterpret_cast<const float4*>(w)[gl + q * G] : zero4();
    const float4* a4 = reinterpret_cast<const float4*>(fa) + pair * HW * C4;
    const float4* b4 = reinterpret_cast<const float4*>(fb) + pair * HW * C4;
    float acc = 0.f;
    for (long base = p0; base < p1; base += NG) {       // uniform trip count: every lane takes part in the butterflies
        const long p = base + g;
        const bool live = p < p1;
        float4 a[HEAD_Q], b[HEAD_Q];
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int q = 0; q < HEAD_Q; ++q) {
            const bool ok = live && gl + q * G < C4;
            a[q] = ok ? a4[p * C4 + gl + q * G] : zero4();
            b[q] = ok ? b4[p * C4 + gl + q * G] : zero4();
            sa += ((a[q].x * a[q].x + a[q].y * a[q].y) + a[q].z * a[q].z) + a[q].w * a[q].w;
            sb += ((b[q].x * b[q].x + b[q].y * b[q].y) + b[q].z * b[q].z) + b[q].w * b[q].w;
        }
        const float na = sqrtf(group_sum<G>(sa)) + 1e-10f, nb = sqrtf(group_sum<G>(sb)) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int q = 0; q < HEAD_Q; ++q) {
            const float dx = a[q].x / na - b[q].x / nb, dy = a[q].y / na - b[q].y / nb;
            const float dz = a[q].z / na - b[q].z / nb, dw = a[q].w / na - b[q].w / nb;
            d += ((wv[q].x * (dx * dx) + wv[q].y * (dy * dy)) + wv[q].z * (dz * dz)) + wv[q].w * (dw * dw);
        }
        d = group_sum<G>(d);
        if (live) acc += d;
    }
    if (gl == 0) red[g] = acc;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int i = 0; i < NG; ++i) s += red[i];
        partial[pair * chunks + chunk] = s;
    }
}

__global__ __launch_bounds__(64) void lpips_finish_kernel(const float* __restrict__ partial, int pairs, int chunks, float count, float* __restrict__ out) {
    const int pair = blockIdx.x * 64 + threadIdx.x;
    if (pair >= pairs) return;
    float s = 0.f;
    for (int i = 0; i < chunks; ++i) s += partial[(long)pair * chunks + i];
    out[pair] = s / count;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int m324_conv3x3(const float* in, const float* wp, const float* bias, float* out, int images, int H, int W, int Cin, int Cout,
                            int relu, void* stream) {
    M324_REQUIRE(in && wp && bias && out, "m324_conv3x3: null in, wp, bias or out");
    M324_REQUIRE(images >= 1 && H >= 1 && W >= 1, "m324_conv3x3: images, H and W must be at least 1, got %d, %d, %d", images, H, W);
    M324_REQUIRE(Cin >= 4 && Cin % 4 == 0, "m324_conv3x3: Cin must be a positive multiple of 4, got %d", Cin);
    M324_REQUIRE(Cout >= 32 && Cout % 32 == 0, "m324_conv3x3: Cout must be a positive multiple of 32, got %d", Cout);
    M324_REQUIRE(Cin <= M324_CONV_MAX_CHANNELS && Cout <= M324_CONV_MAX_CHANNELS, "m324_conv3x3: at most %d channels, got Cin %d, Cout %d",
                 M324_CONV_MAX_CHANNELS, Cin, Cout);
    const long M = (long)images * H * W;
    M324_REQUIRE(M <= 0x7fffffffL && (long)H * W <= 0x7fffffffL, "m324_conv3x3: images * H * W must stay below 2^31, got %ld", M);
    M324_REQUIRE(aligned16(in) && aligned16(wp) && aligned16(out), "m324_conv3x3: in, wp and out must be 16-byte aligned");
    M324_REQUIRE(relu == 0 || relu == 1, "m324_conv3x3: relu is 0 or 1, got %d", relu);
    const int K = 9 * Cin;
    const long m_tiles = (M + BM - 1) / BM;
    hipStream_t st = (hipStream_t)stream;
    if (Cout % 128 == 0) {
        const int n_tiles = Cout / 128;
        hipLaunchKernelGGL(conv3x3_kernel<128>, dim3((unsigned)(m_tiles * n_tiles)), dim3(THREADS), 0, st, in, wp, bias, out, M, H, W, Cin, Cout, K,
                           n_tiles, relu);
    } else {
        const int n_tiles = (Cout + 63) / 64;
        hipLaunchKernelGGL(conv3x3_kernel<64>, dim3((unsigned)(m_tiles * n_tiles)), dim3(THREADS), 0, st, in, wp, bias, out, M, H, W, Cin, Cout, K,
                           n_tiles, relu);
    }
    M324_CHECK_LAUNCH("m324_conv3x3");
    return M324_OK;
}

extern "C" int m324_maxpool2x2(const float* in, float* out, int images, int H, int W, int C, void* stream) {
    M324_REQUIRE(in && out, "m324_maxpool2x2: null in or out");
    M324_REQUIRE(images >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "m324_maxpool2x2: images >= 1 and even H, W >= 2, got %d, %d, %d",
                 images, H, W);
    M324_REQUIRE(C >= 4 && C % 4 == 0 && C <= M324_CONV_MAX_CHANNELS, "m324_maxpool2x2: C must be a multiple of 4 in 4..%d, got %d",
                 M324_CONV_MAX_CHANNELS, C);
    M324_REQUIRE((long)images * H * W <= 0x7fffffffL, "m324_maxpool2x2: images * H * W must stay below 2^31");
    M324_REQUIRE(aligned16(in) && aligned16(out), "m324_maxpool2x2: in and out must be 16-byte aligned");
    const long total = (long)images * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                       (const float4*)in, (float4*)out, total, H / 2, W / 2, C / 4);
    M324_CHECK_LAUNCH("m324_maxpool2x2");
    return M324_OK;
}

extern "C" int m324_lpips_prepare(const void* src, int mode, int normalize, int images, int H, int W, float* dst, void* stream) {
    M324_REQUIRE(src && dst, "m324_lpips_prepare: null src or dst");
    M324_REQUIRE(mode == M324_LPIPS_U8_NHWC || mode == M324_LPIPS_F32_NCHW, "m324_lpips_prepare: unknown mode %d", mode);
    M324_REQUIRE(normalize == 0 || (normalize == 1 && mode == M324_LPIPS_F32_NCHW),
                 "m324_lpips_prepare: normalize is 0, or 1 with fp32 input, got %d with mode %d", normalize, mode);
    M324_REQUIRE(images >= 1 && H >= 1 && W >= 1 && (long)images * H * W <= 0x7fffffffL,
                 "m324_lpips_prepare: images, H, W >= 1 and images * H * W below 2^31, got %d, %d, %d", images, H, W);
    M324_REQUIRE(aligned16(dst) && (mode == M324_LPIPS_U8_NHWC || ((uintptr_t)src & 3) == 0), "m324_lpips_prepare: dst must be 16-byte, fp32 src 4-byte aligned");
    const long HW = (long)H * W, total = images * HW;
    hipLaunchKernelGGL(lpips_prepare_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, src, mode,
                       normalize, total, HW, (float4*)dst);
    M324_CHECK_LAUNCH("m324_lpips_prepare");
    return M324_OK;
}

extern "C" int m324_lpips_layer(const float* fa, const float* fb, const float* w, int pairs, long pixels, int channels, float* partial,
                                float* out, void* stream) {
    M324_REQUIRE(fa && fb && w && partial && out, "m324_lpips_layer: null fa, fb, w, partial or out");
    M324_REQUIRE(pairs >= 1 && pixels >= 1 && pixels <= (1L << 24), "m324_lpips_layer: pairs >= 1 and 1 <= pixels <= 2^24, got %d, %ld", pairs, pixels);
    M324_REQUIRE(channels >= 4 && channels % 4 == 0 && channels <= M324_LPIPS_MAX_CHANNELS,
                 "m324_lpips_layer: channels must be a multiple of 4 in 4..%d, got %d", M324_LPIPS_MAX_CHANNELS, channels);
    M324_REQUIRE((long)pairs * pixels <= 0x7fffffffL, "m324_lpips_layer: pairs * pixels must stay below 2^31");
    M324_REQUIRE(aligned16(fa) && aligned16(fb) && aligned16(w), "m324_lpips_layer: fa, fb and w must be 16-byte aligned");
    const long by64 = (pixels + 63) / 64;
    const int chunks = (int)(by64 < M324_LPIPS_CHUNKS ? by64 : M324_LPIPS_CHUNKS);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long)pairs * chunks));
    const int c4 = channels / 4;
    static_assert(M324_LPIPS_MAX_CHANNELS == 64 * 4 * 4, "the widest head kernel holds four 16-byte pieces per lane");
    if (c4 <= 16)
        hipLaunchKernelGGL((lpips_layer_kernel<16, 1>), grid, dim3(THREADS), 0, st, fa, fb, w, pixels, channels, chunks, partial);
    else if (c4 <= 32)
        hipLaunchKernelGGL((lpips_layer_kernel<32, 1>), grid, dim3(THREADS), 0, st, fa, fb, w, pixels, channels, chunks, partial);
    else if (c4 <= 64)
        hipLaunchKernelGGL((lpips_layer_kernel<64, 1>), grid, dim3(THREADS), 0, st, fa, fb, w, pixels, channels, chunks, partial);
    else if (c4 <= 128)
        hipLaunchKernelGGL((lpips_layer_kernel<64, 2>), grid, dim3(THREADS), 0, st, fa, fb, w, pixels, channels, chunks, partial);
    else
        hipLaunchKernelGGL((lpips_layer_kernel<64, 4>), grid, dim3(THREADS), 0, st, fa, fb, w, pixels, channels, chunks, partial);
    M324_CHECK_LAUNCH("m324_lpips_layer");
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, st, partial, pairs, chunks, (float)pixels, out);
    M324_CHECK_LAUNCH("m324_lpips_layer");
    return M324_OK;
}
