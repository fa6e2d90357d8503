// Perceptual evaluation (LPIPS on a VGG16 trunk): the input scaling and the normalise-subtract-square-weigh head.  The trunk's
// 3 x 3 convolution and 2 x 2 max-pool are in csrc/conv.hip.  The contract of every entry point is in include/m324.h; what is
// here is how.
#include "common.h"
#include <math.h>

namespace {

constexpr int THREADS = 256;

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

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
