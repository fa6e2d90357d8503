// Foreground matting (U2-Net and ISNet): the bilinear upsample, the input normalisation, the fused side-output head of U2-Net, the
// one-map head of ISNet and the quantisation of the matte.  The networks' 3 x 3 convolutions and their ceil-mode pool are in csrc/conv.hip.  The contract of every entry point
// is in include/m324.h; what is here is how.
#include "common.h"
#include <math.h>

namespace {

constexpr int THREADS = 256;

// one axis of the bilinear resize (align_corners = false): the two source samples of output o and their weights
struct Lerp {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Lerp lerp_of(int o, int in, int out) {
#pragma clang fp contract(off)
    const float scale = (float)in / (float)out;
    float s = ((float)o + 0.5f) * scale - 0.5f;
    s = s < 0.f ? 0.f : s;
    Lerp r;
    r.i0 = (int)s;
    r.i0 = r.i0 > in - 1 ? in - 1 : r.i0;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = fminf(fmaxf(s - (float)r.i0, 0.f), 1.f);
    r.l0 = 1.0f - r.l1;
    return r;
}

__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, const Lerp& y, const Lerp& x) {
#pragma clang fp contract(off)
    return y.l0 * (x.l0 * v00 + x.l1 * v01) + y.l1 * (x.l0 * v10 + x.l1 * v11);
}

__global__ __launch_bounds__(THREADS) void upsample_bilinear_kernel(const float4* __restrict__ in, float4* __restrict__ out, long total, int H, int W,
                                                                    int Ho, int Wo, int C4) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    long r = i / C4;
    const int x = (int)(r % Wo);
    r /= Wo;
    const int y = (int)(r % Ho);
    const long img = r / Ho;
    const Lerp ly = lerp_of(y, H, Ho), lx = lerp_of(x, W, Wo);
    const float4* s = in + img * H * W * C4 + c;
    const float4 v00 = s[((long)ly.i0 * W + lx.i0) * C4], v01 = s[((long)ly.i0 * W + lx.i1) * C4];
    const float4 v10 = s[((long)ly.i1 * W + lx.i0) * C4], v11 = s[((long)ly.i1 * W + lx.i1) * C4];
    out[i] = make_float4(bilerp(v00.x, v01.x, v10.x, v11.x, ly, lx), bilerp(v00.y, v01.y, v10.y, v11.y, ly, lx),
                         bilerp(v00.z, v01.z, v10.z, v11.z, ly, lx), bilerp(v00.w, v01.w, v10.w, v11.w, ly, lx));
}

// The per-frame reductions have two levels so that a clip of a few frames still fills the chip: a frame is cut into `chunks` equal
// runs, a workgroup reduces one run, and a second kernel reduces a frame's runs.  Maxima and minima are exact in any order.
int chunks_of(long n) {
    const long c = (n + M324_MATTE_CHUNK_ITEMS - 1) / M324_MATTE_CHUNK_ITEMS;
    return (int)(c < M324_MATTE_CHUNKS ? c : M324_MATTE_CHUNKS);
}

// the largest byte of every run of every frame
__global__ __launch_bounds__(THREADS) void frame_bytemax_kernel(const unsigned char* __restrict__ src, long bytes, int chunks, int* __restrict__ partial) {
    __shared__ int red[THREADS];
    const long frame = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const long per = (bytes + chunks - 1) / chunks;
    const long p0 = chunk * per, p1 = p0 + per < bytes ? p0 + per : bytes;
    const unsigned char* s = src + frame * bytes;
    int m = 0;
    for (long i = p0 + threadIdx.x; i < p1; i += THREADS) m = max(m, (int)s[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void frame_bytemax_finish_kernel(const int* __restrict__ partial, int images, int chunks, int* __restrict__ frame_max) {
    const int img = blockIdx.x * 64 + threadIdx.x;
    if (img >= images) return;
    int m = 0;
    for (int i = 0; i < chunks; ++i) m = max(m, partial[(long)img * chunks + i]);
    frame_max[img] = m;
}

struct MeanStd {
    double mean[3], std[3];
};

// x_c = (v_c / m - mean_c) / std_c in float64, rounded once to fp32: what numpy computes for the same bytes.  The constants are
// arguments (U2-Net's session and the DIS session of `rembg` differ in them); an IEEE division by a number known only at run time
// has the bits of the division by the same literal.
__global__ __launch_bounds__(THREADS) void matte_prepare_kernel(const unsigned char* __restrict__ src, const int* __restrict__ frame_max, long total,
                                                                long HW, MeanStd c, float4* __restrict__ dst) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int fm = frame_max[i / HW];
    const double m = fm > 0 ? (double)fm : 1e-6;
    const unsigned char* s = src + 3 * i;
    const double x0 = ((double)s[0] / m - c.mean[0]) / c.std[0], x1 = ((double)s[1] / m - c.mean[1]) / c.std[1],
                 x2 = ((double)s[2] / m - c.mean[2]) / c.std[2];
    dst[i] = make_float4((float)x0, (float)x1, (float)x2, 0.f);
}

struct FuseArgs {
    const float* side[M324_MATTE_SIDES];
    int h[M324_MATTE_SIDES], w[M324_MATTE_SIDES];
    float weight[M324_MATTE_SIDES];
    float bias;
};

__global__ __launch_bounds__(THREADS) void matte_fuse_kernel(FuseArgs fa, int stride, long total, int Ho, int Wo, float* __restrict__ prob,
                                                             float* __restrict__ logit) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % Wo);
    const long r = i / Wo;
    const int y = (int)(r % Ho);
    const long img = r / Ho;
    float d0 = 0.f;
#pragma unroll
    for (int k = 0; k < M324_MATTE_SIDES; ++k) {
        const int h = fa.h[k], w = fa.w[k];
        const Lerp ly = lerp_of(y, h, Ho), lx = lerp_of(x, w, Wo);
        const float* s = fa.side[k] + img * h * w * stride;
        const float v = bilerp(s[((long)ly.i0 * w + lx.i0) * stride], s[((long)ly.i0 * w + lx.i1) * stride],
                               s[((long)ly.i1 * w + lx.i0) * stride], s[((long)ly.i1 * w + lx.i1) * stride], ly, lx);
        d0 = d0 + fa.weight[k] * v;
    }
    d0 = d0 + fa.bias;
    if (logit) logit[i] = d0;
    prob[i] = 1.0f / (1.0f + expf(-d0));
}

// ISNet's head: the one side map sampled at the output's pixel, then the sigmoid; the upsampled map itself is never written
__global__ __launch_bounds__(THREADS) void matte_side_kernel(const float* __restrict__ side, int h, int w, int stride, long total, int Ho, int Wo,
                                                             float* __restrict__ prob, float* __restrict__ logit) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % Wo);
    const long r = i / Wo;
    const int y = (int)(r % Ho);
    const long img = r / Ho;
    const Lerp ly = lerp_of(y, h, Ho), lx = lerp_of(x, w, Wo);
    const float* s = side + img * h * w * stride;
    const float d1 = bilerp(s[((long)ly.i0 * w + lx.i0) * stride], s[((long)ly.i0 * w + lx.i1) * stride], s[((long)ly.i1 * w + lx.i0) * stride],
                            s[((long)ly.i1 * w + lx.i1) * stride], ly, lx);
    if (logit) logit[i] = d1;
    prob[i] = 1.0f / (1.0f + expf(-d1));
}

// the smallest and the largest value of every run of every frame
__global__ __launch_bounds__(THREADS) void frame_minmax_kernel(const float* __restrict__ p, long pixels, int chunks, float* __restrict__ partial) {
    __shared__ float lo[THREADS], hi[THREADS];
    const long frame = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const long per = (pixels + chunks - 1) / chunks;
    const long p0 = chunk * per, p1 = p0 + per < pixels ? p0 + per : pixels;
    const float* s = p + frame * pixels;
    float a = INFINITY, b = -INFINITY;
    for (long i = p0 + threadIdx.x; i < p1; i += THREADS) {
        const float v = s[i];
        a = fminf(a, v);
        b = fmaxf(b, v);
    }
    lo[threadIdx.x] = a;
    hi[threadIdx.x] = b;
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            lo[threadIdx.x] = fminf(lo[threadIdx.x], lo[threadIdx.x + off]);
            hi[threadIdx.x] = fmaxf(hi[threadIdx.x], hi[threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2L * blockIdx.x] = lo[0];
        partial[2L * blockIdx.x + 1] = hi[0];
    }
}

__global__ __launch_bounds__(64) void frame_minmax_finish_kernel(const float* __restrict__ partial, int images, int chunks, float* __restrict__ minmax) {
    const int img = blockIdx.x * 64 + threadIdx.x;
    if (img >= images) return;
    float a = INFINITY, b = -INFINITY;
    for (int i = 0; i < chunks; ++i) {
        a = fminf(a, partial[2 * ((long)img * chunks + i)]);
        b = fmaxf(b, partial[2 * ((long)img * chunks + i) + 1]);
    }
    minmax[2 * img] = a;
    minmax[2 * img + 1] = b;
}

__global__ __launch_bounds__(THREADS) void matte_quantise_kernel(const float* __restrict__ p, const float* __restrict__ minmax, long total, long pixels,
                                                                 unsigned char* __restrict__ q) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const long img = i / pixels;
    const float mi = minmax[2 * img], ma = minmax[2 * img + 1];
    float v = 0.f;
    if (ma > mi) v = ((p[i] - mi) / (ma - mi)) * 255.0f;
    v = v >= 0.f ? v : 0.f;                         // also a NaN input
    q[i] = (unsigned char)(v > 255.f ? 255.f : v);  // truncation, as numpy's astype(uint8)
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned blocks_of(long total) { return (unsigned)((total + THREADS - 1) / THREADS); }

}  // namespace

extern "C" int m324_upsample_bilinear(const float* in, float* out, int images, int H, int W, int Ho, int Wo, int C, void* stream) {
    M324_REQUIRE(in && out, "m324_upsample_bilinear: null in or out");
    M324_REQUIRE(images >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "m324_upsample_bilinear: images and all sizes must be at least 1, got %d, %d x %d -> %d x %d",
                 images, H, W, Ho, Wo);
    M324_REQUIRE(H <= M324_MATTE_MAX_SIDE && W <= M324_MATTE_MAX_SIDE && Ho <= M324_MATTE_MAX_SIDE && Wo <= M324_MATTE_MAX_SIDE,
                 "m324_upsample_bilinear: sizes up to %d, got %d x %d -> %d x %d", M324_MATTE_MAX_SIDE, H, W, Ho, Wo);
    M324_REQUIRE(C >= 4 && C % 4 == 0 && C <= M324_CONV_MAX_CHANNELS, "m324_upsample_bilinear: C must be a multiple of 4 in 4..%d, got %d",
                 M324_CONV_MAX_CHANNELS, C);
    M324_REQUIRE((long)images * H * W <= 0x7fffffffL && (long)images * Ho * Wo <= 0x7fffffffL,
                 "m324_upsample_bilinear: images * H * W and images * Ho * Wo must stay below 2^31");
    M324_REQUIRE(aligned16(in) && aligned16(out), "m324_upsample_bilinear: in and out must be 16-byte aligned");
    const long total = (long)images * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(upsample_bilinear_kernel, dim3(blocks_of(total)), dim3(THREADS), 0, (hipStream_t)stream, (const float4*)in, (float4*)out, total,
                       H, W, Ho, Wo, C / 4);
    M324_CHECK_LAUNCH("m324_upsample_bilinear");
    return M324_OK;
}

namespace {

// both entry points of the normalisation: the contract, then the three launches
int matte_prepare(const char* name, const unsigned char* src, int images, int H, int W, const double* mean_std, int* partial, int* frame_max,
                  float* dst, void* stream) {
    M324_REQUIRE(src && partial && frame_max && dst, "%s: null src, partial, frame_max or dst", name);
    M324_REQUIRE(images >= 1 && H >= 1 && W >= 1 && (long)images * H * W <= 0x7fffffffL,
                 "%s: images, H, W >= 1 and images * H * W below 2^31, got %d, %d, %d", name, images, H, W);
    M324_REQUIRE(aligned16(dst) && (((uintptr_t)frame_max | (uintptr_t)partial) & 3) == 0,
                 "%s: dst must be 16-byte, partial and frame_max 4-byte aligned", name);
    MeanStd c;
    for (int k = 0; k < 3; ++k) {
        M324_REQUIRE(isfinite(mean_std[k]), "%s: mean %d is not finite", name, k);
        M324_REQUIRE(isfinite(mean_std[3 + k]) && mean_std[3 + k] > 0.0, "%s: std %d must be finite and above 0, got %g", name, k, mean_std[3 + k]);
        c.mean[k] = mean_std[k];
        c.std[k] = mean_std[3 + k];
    }
    const long HW = (long)H * W, total = images * HW;
    hipStream_t st = (hipStream_t)stream;
    const int chunks = chunks_of(3 * HW);
    hipLaunchKernelGGL(frame_bytemax_kernel, dim3((unsigned)((long)images * chunks)), dim3(THREADS), 0, st, src, 3 * HW, chunks, partial);
    M324_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(frame_bytemax_finish_kernel, dim3((unsigned)((images + 63) / 64)), dim3(64), 0, st, (const int*)partial, images, chunks, frame_max);
    M324_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(matte_prepare_kernel, dim3(blocks_of(total)), dim3(THREADS), 0, st, src, (const int*)frame_max, total, HW, c, (float4*)dst);
    M324_CHECK_LAUNCH(name);
    return M324_OK;
}

}  // namespace

extern "C" int m324_matte_prepare(const unsigned char* src, int images, int H, int W, int* partial, int* frame_max, float* dst, void* stream) {
    static const double imagenet[6] = {0.485, 0.456, 0.406, 0.229, 0.224, 0.225};
    return matte_prepare("m324_matte_prepare", src, images, H, W, imagenet, partial, frame_max, dst, stream);
}

extern "C" int m324_matte_prepare_ex(const unsigned char* src, int images, int H, int W, const double* mean_std, int* partial, int* frame_max,
                                     float* dst, void* stream) {
    M324_REQUIRE(mean_std, "m324_matte_prepare_ex: null mean_std");
    return matte_prepare("m324_matte_prepare_ex", src, images, H, W, mean_std, partial, frame_max, dst, stream);
}

extern "C" int m324_matte_side(const float* side, int side_h, int side_w, int side_stride, int images, int Ho, int Wo, float* prob, float* logit,
                               void* stream) {
    M324_REQUIRE(side && prob, "m324_matte_side: null side or prob");
    M324_REQUIRE(images >= 1 && Ho >= 1 && Wo >= 1 && Ho <= M324_MATTE_MAX_SIDE && Wo <= M324_MATTE_MAX_SIDE && (long)images * Ho * Wo <= 0x7fffffffL,
                 "m324_matte_side: images >= 1, Ho and Wo in 1..%d, images * Ho * Wo below 2^31, got %d, %d, %d", M324_MATTE_MAX_SIDE, images, Ho, Wo);
    M324_REQUIRE(side_stride >= 1 && side_stride <= M324_CONV_MAX_CHANNELS, "m324_matte_side: side_stride must be in 1..%d, got %d",
                 M324_CONV_MAX_CHANNELS, side_stride);
    M324_REQUIRE(side_h >= 1 && side_w >= 1 && side_h <= Ho && side_w <= Wo,
                 "m324_matte_side: the side map must be between 1 x 1 and the output's %d x %d, got %d x %d", Ho, Wo, side_h, side_w);
    M324_REQUIRE((((uintptr_t)side | (uintptr_t)prob | (uintptr_t)logit) & 3) == 0, "m324_matte_side: side, prob and logit must be 4-byte aligned");
    const long total = (long)images * Ho * Wo;
    hipLaunchKernelGGL(matte_side_kernel, dim3(blocks_of(total)), dim3(THREADS), 0, (hipStream_t)stream, side, side_h, side_w, side_stride, total, Ho, Wo,
                       prob, logit);
    M324_CHECK_LAUNCH("m324_matte_side");
    return M324_OK;
}

extern "C" int m324_matte_fuse(const float* const* sides, const int* side_h, const int* side_w, int side_stride, const float* outconv, int images,
                               int Ho, int Wo, float* prob, float* logit, void* stream) {
    M324_REQUIRE(sides && side_h && side_w && outconv && prob, "m324_matte_fuse: null sides, side_h, side_w, outconv or prob");
    M324_REQUIRE(images >= 1 && Ho >= 1 && Wo >= 1 && Ho <= M324_MATTE_MAX_SIDE && Wo <= M324_MATTE_MAX_SIDE && (long)images * Ho * Wo <= 0x7fffffffL,
                 "m324_matte_fuse: images >= 1, Ho and Wo in 1..%d, images * Ho * Wo below 2^31, got %d, %d, %d", M324_MATTE_MAX_SIDE, images, Ho, Wo);
    M324_REQUIRE(side_stride >= 1 && side_stride <= M324_CONV_MAX_CHANNELS, "m324_matte_fuse: side_stride must be in 1..%d, got %d",
                 M324_CONV_MAX_CHANNELS, side_stride);
    M324_REQUIRE((((uintptr_t)prob | (uintptr_t)logit) & 3) == 0, "m324_matte_fuse: prob and logit must be 4-byte aligned");
    FuseArgs fa;
    for (int k = 0; k < M324_MATTE_SIDES; ++k) {
        M324_REQUIRE(sides[k] && ((uintptr_t)sides[k] & 3) == 0, "m324_matte_fuse: side map %d is null or not 4-byte aligned", k);
        M324_REQUIRE(side_h[k] >= 1 && side_w[k] >= 1 && side_h[k] <= Ho && side_w[k] <= Wo,
                     "m324_matte_fuse: side map %d must be between 1 x 1 and the output's %d x %d, got %d x %d", k, Ho, Wo, side_h[k], side_w[k]);
        M324_REQUIRE(isfinite(outconv[k]), "m324_matte_fuse: outconv weight %d is not finite", k);
        fa.side[k] = sides[k];
        fa.h[k] = side_h[k];
        fa.w[k] = side_w[k];
        fa.weight[k] = outconv[k];
    }
    M324_REQUIRE(isfinite(outconv[M324_MATTE_SIDES]), "m324_matte_fuse: the outconv bias is not finite");
    fa.bias = outconv[M324_MATTE_SIDES];
    const long total = (long)images * Ho * Wo;
    hipLaunchKernelGGL(matte_fuse_kernel, dim3(blocks_of(total)), dim3(THREADS), 0, (hipStream_t)stream, fa, side_stride, total, Ho, Wo, prob, logit);
    M324_CHECK_LAUNCH("m324_matte_fuse");
    return M324_OK;
}

extern "C" int m324_matte_quantise(const float* p, int images, long pixels, float* partial, float* minmax, unsigned char* q, void* stream) {
    M324_REQUIRE(p && partial && minmax && q, "m324_matte_quantise: null p, partial, minmax or q");
    M324_REQUIRE(images >= 1 && pixels >= 1 && (long)images * pixels <= 0x7fffffffL && pixels <= 0x7fffffffL,
                 "m324_matte_quantise: images, pixels >= 1 and images * pixels below 2^31, got %d, %ld", images, pixels);
    M324_REQUIRE((((uintptr_t)p | (uintptr_t)partial | (uintptr_t)minmax) & 3) == 0, "m324_matte_quantise: p, partial and minmax must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int chunks = chunks_of(pixels);
    hipLaunchKernelGGL(frame_minmax_kernel, dim3((unsigned)((long)images * chunks)), dim3(THREADS), 0, st, p, pixels, chunks, partial);
    M324_CHECK_LAUNCH("m324_matte_quantise");
    hipLaunchKernelGGL(frame_minmax_finish_kernel, dim3((unsigned)((images + 63) / 64)), dim3(64), 0, st, (const float*)partial, images, chunks, minmax);
    M324_CHECK_LAUNCH("m324_matte_quantise");
    const long total = images * pixels;
    hipLaunchKernelGGL(matte_quantise_kernel, dim3(blocks_of(total)), dim3(THREADS), 0, st, p, (const float*)minmax, total, pixels, q);
    M324_CHECK_LAUNCH("m324_matte_quantise");
    return M324_OK;
}
