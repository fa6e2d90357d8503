// Kernels of a plain ViT image tower in fp32 (open_clip's VisionTransformer, motion324_amd/clipsim.py): self-attention at any
// head width D % 8 == 0 up to 128 read straight from the token-major q|k|v rows of a fused in-projection, a LayerNorm for rows
// up to 4096 wide, the patch rows of ToTensor + Normalize, and the class token / positional embedding assembly.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------- attention
// A plain descendant of attn_f32_kernel (attention.hip): four waves of 32 queries, S^T = K Q^T and O^T += V^T P^T on
// v_mfma_f32_32x32x2_f32, the online softmax in the log2 domain.  What differs: the head width is a template parameter
// (DP = D rounded up to 32; columns D..DP-1 of q, k, v are zeros, which add exact zeros to every product), q, k and v come from
// one row of the in-projection's output, and V is staged row-major as it is read: the P V step takes V[key][d] with d across the
// lanes, so consecutive lanes read consecutive words of one padded row and no transpose is needed.
constexpr int TOK_QW = 32;            // query rows per wave
constexpr int TOK_NW = 4;             // waves per workgroup
constexpr int TOK_QB = TOK_QW * TOK_NW;

template <int DP, int KT>             // KT keys per tile: 64, or 32 at DP = 128 (two 64-key tiles of 129 floats would be 66 KB)
__global__ __launch_bounds__(256) void attn_tok_kernel(const float* __restrict__ qkv, long ld, float* __restrict__ O, long ldo,
                                                       int L, int H, int D, float scale_log2e) {
    constexpr int LD = DP + 1;        // padded row length (floats): conflict-free column reads of K
    constexpr int C4 = DP / 4;        // float4 pieces per staged row
    constexpr int KB = KT / 32, DB = DP / 32;
    __shared__ float sk[KT * LD];     // [key][d]
    __shared__ float sv[KT * LD];     // [key][d]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y;
    const int q0 = blockIdx.x * TOK_QB + wave * TOK_QW;
    const long HD = (long)H * D;
    const float* base = qkv + (long)b * L * ld + (long)h * D;      // q of token 0; k at + HD, v at + 2 HD

    // lane (q, hi) holds Q[q][2s + hi], s = 0..DP/2-1
    float qf[DP / 2];
    {
        const int q = q0 + l31;
        const bool ok = q < L;
        const float* qr = base + (long)(ok ? q : 0) * ld;
#pragma unroll
        for (int s = 0; s < DP / 2; ++s) qf[s] = (ok && 2 * s < D) ? qr[2 * s + hi] : 0.f;
    }
    f32x16 o[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int nt = (L + KT - 1) / KT;
    for (int t = 0; t < nt; ++t) {
        const int kv0 = t * KT;
        __syncthreads();   // previous tile fully consumed
        for (int id = tid; id < KT * C4; id += 256) {
            const int row = id / C4, c = id - row * C4;
            float4 kx = make_float4(0.f, 0.f, 0.f, 0.f), vx = kx;
            if (kv0 + row < L && c * 4 < D) {                       // keys >= L and columns >= D are zeros
                const float* kr = base + (long)(kv0 + row) * ld + HD + c * 4;
                kx = *reinterpret_cast<const float4*>(kr);
                vx = *reinterpret_cast<const float4*>(kr + HD);
            }
            float* pk = sk + row * LD + c * 4;
            float* pv = sv + row * LD + c * 4;
            pk[0] = kx.x; pk[1] = kx.y; pk[2] = kx.z; pk[3] = kx.w;
            pv[0] = vx.x; pv[1] = vx.y; pv[2] = vx.z; pv[3] = vx.w;
        }
        __syncthreads();

        f32x16 s[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
            for (int st = 0; st < DP / 2; ++st)
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(sk[(kb * 32 + l31) * LD + 2 * st + hi], qf[st], s[kb], 0, 0, 0);
        }
        if (kv0 + KT > L) {   // ragged last tile: the scores of the keys >= L become -inf (tile 0 always holds key 0)
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kv0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi >= L) s[kb][r] = -INFINITY;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // scale > 0 (checked by the entry point), so the maximum of the scaled scores is the scaled maximum
        const float m_new = fmaxf(m_run, mx * scale_log2e);
        const float alpha = exp2f(m_run - m_new);
        m_run = m_new;
        float rs = 0.f;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[kb][r] = exp2f(fmaf(s[kb][r], scale_log2e, -m_new));
                rs += s[kb][r];
            }
        l_run = l_run * alpha + rs;
#pragma unroll
        for (int i = 0; i < DB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
        // O^T += V^T P^T : MFMA step (kb, r) contracts key kv = kb*32 + (r&3) + 8*(r>>2) + 4*hi; lane (d, hi) supplies V[kv][d]
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kv = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
#pragma unroll
                for (int db = 0; db < DB; ++db)
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv[kv * LD + db * 32 + l31], s[kb][r], o[db], 0, 0, 0);
            }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    const int q = q0 + l31;
    if (q < L) {
        float* orow = O + ((long)b * L + q) * ldo + (long)h * D;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = db * 32 + g * 8 + hi * 4;             // D % 8 == 0: a group of four is inside or outside as a whole
                if (d < D)
                    *reinterpret_cast<float4*>(orow + d) = make_float4(o[db][g * 4 + 0] * inv, o[db][g * 4 + 1] * inv,
                                                                       o[db][g * 4 + 2] * inv, o[db][g * 4 + 3] * inv);
            }
    }
}

// ------------------------------------------------------------------------------------------- layernorm
// One wave per row, four rows per workgroup; the row is read three times (mean, squared deviations, output) in float4 pieces,
// the second and third time from cache.  Same arithmetic as m324_layernorm: mean first, then the sum of squared deviations.
__global__ __launch_bounds__(256) void layernorm_wide_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ w,
                                                             const float* __restrict__ b, float eps, float* __restrict__ y, long ldy,
                                                             int rows, int C) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * ldx;
    float s = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + c);
        s += v.x + v.y + v.z + v.w;
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + c);
        const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
        q += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    float* yr = y + row * ldy;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + c);
        const float4 ww = *reinterpret_cast<const float4*>(w + c);
        const float4 bb = b ? *reinterpret_cast<const float4*>(b + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(yr + c) = make_float4((v.x - mean) * rstd * ww.x + bb.x, (v.y - mean) * rstd * ww.y + bb.y,
                                                         (v.z - mean) * rstd * ww.z + bb.z, (v.w - mean) * rstd * ww.w + bb.w);
    }
}

// ------------------------------------------------------------------------------------------- patch rows
// One thread per output element; consecutive threads write consecutive columns of one patch row.
__global__ __launch_bounds__(256) void vit_patches_kernel(const unsigned char* __restrict__ img, int S, int patch, int g,
                                                          const float* __restrict__ mean_std, float* __restrict__ out, int Kp, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long row = i / Kp;
    const int col = (int)(i - row * Kp);
    const int pp = patch * patch;
    float v = 0.f;
    if (col < 3 * pp) {
        const int c = col / pp, k = col - c * pp, ky = k / patch, kx = k - ky * patch;
        const long f = row / (g * g);
        const int p = (int)(row - f * g * g), py = p / g, px = p - py * g;
        const unsigned char u = img[((f * S + py * patch + ky) * S + px * patch + kx) * 3 + c];
        v = __fdiv_rn(__fsub_rn(__fdiv_rn((float)u, 255.0f), mean_std[c]), mean_std[3 + c]);
    }
    out[i] = v;
}

__global__ __launch_bounds__(256) void vit_tokens_kernel(const float* __restrict__ patch_rows, const float* __restrict__ cls,
                                                         const float* __restrict__ pos, float* __restrict__ x, int L, int C4, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;           // one float4 of x
    if (i >= total) return;
    const long row = i / C4;
    const int c = (int)(i - row * C4) * 4;
    const long f = row / L;
    const int l = (int)(row - f * L);
    const long C = (long)C4 * 4;
    const float4 a = *reinterpret_cast<const float4*>(l == 0 ? cls + c : patch_rows + (f * (L - 1) + (l - 1)) * C + c);
    const float4 p = *reinterpret_cast<const float4*>(pos + (long)l * C + c);
    *reinterpret_cast<float4*>(x + row * C + c) = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
}

// ------------------------------------------------------------------------------------------- float resize
// One separable pass under host-built tables (motion324_amd/dreamsim.py resize_tables).  Every form runs the same chain per
// output -- acc = fmaf(w[k], sample(first + k), acc) in tap order -- so which form a shape takes never shows in the result.
// A byte sample is (float)v / 255, one IEEE division (ToTensor).  `first` is clamped into the axis and taps at or past its end
// are skipped: no table can make a read leave the source.
__device__ __forceinline__ float byte_sample(unsigned v) { return __fdiv_rn((float)v, 255.0f); }

// source element (f, c, y, x) of either form
template <bool U8>
__device__ __forceinline__ float src_at(const void* src, long f, int c, int y, int x, int H, int W) {
    if constexpr (U8) return byte_sample(static_cast<const unsigned char*>(src)[((f * H + y) * W + x) * 3 + c]);
    else return static_cast<const float*>(src)[((f * 3 + c) * H + y) * W + x];
}

// any shape: one thread per output element, consecutive threads along the output row
template <bool U8, int AXIS>
__global__ __launch_bounds__(256) void resample_scalar_kernel(const void* __restrict__ src, int H, int W, const float* __restrict__ wt,
                                                              const int* __restrict__ first, int ksize, int n_out,
                                                              float* __restrict__ dst, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int OW = AXIS == 0 ? n_out : W, OH = AXIS == 0 ? H : n_out, n_in = AXIS == 0 ? W : H;
    const int ox = (int)(i % OW);
    const long r = i / OW;
    const int oy = (int)(r % OH);
    const long fc = r / OH;
    const int c = (int)(fc % 3);
    const long f = fc / 3;
    const int o = AXIS == 0 ? ox : oy;
    const int j0 = min(max(first[o], 0), n_in - 1);
    const float* w = wt + (long)o * ksize;
    float acc = 0.f;
    for (int k = 0; k < ksize && j0 + k < n_in; ++k)
        acc = fmaf(w[k], AXIS == 0 ? src_at<U8>(src, f, c, oy, j0 + k, H, W) : src_at<U8>(src, f, c, j0 + k, ox, H, W), acc);
    dst[i] = acc;
}

// x pass, n_out % 4 == 0: one thread per four consecutive outputs of a row, one 16-byte store.  The taps are gathers (a lane's
// four windows start scale pixels apart and are not aligned to anything); neighbouring lanes read neighbouring windows of the
// same source row, so a wave's reads of one tap step fall into a few consecutive cache lines.
template <bool U8>
__global__ __launch_bounds__(256) void resample_x4_kernel(const void* __restrict__ src, int H, int W, const float* __restrict__ wt,
                                                          const int* __restrict__ first, int ksize, int n_out,
                                                          float* __restrict__ dst, long total4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;           // one float4 of dst
    if (i >= total4) return;
    const int O4 = n_out >> 2;
    const int o0 = (int)(i % O4) * 4;
    const long r = i / O4;
    const int y = (int)(r % H);
    const long fc = r / H;
    const int c = (int)(fc % 3);
    const long f = fc / 3;
    float acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j0 = min(max(first[o0 + e], 0), W - 1);
        const float* w = wt + (long)(o0 + e) * ksize;
        float a = 0.f;
        for (int k = 0; k < ksize && j0 + k < W; ++k) a = fmaf(w[k], src_at<U8>(src, f, c, y, j0 + k, H, W), a);
        acc[e] = a;
    }
    *reinterpret_cast<float4*>(dst + i * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// y pass over fp32 planes, W % 4 == 0: one thread per four consecutive columns; every tap is a 16-byte load from a source row and
// consecutive lanes read consecutive 16 bytes of it
__global__ __launch_bounds__(256) void resample_y4_f32_kernel(const float* __restrict__ src, int H, int W, const float* __restrict__ wt,
                                                              const int* __restrict__ first, int ksize, int n_out,
                                                              float* __restrict__ dst, long total4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int W4 = W >> 2;
    const int x = (int)(i % W4) * 4;
    const long r = i / W4;
    const int oy = (int)(r % n_out);
    const long fc = r / n_out;
    const int j0 = min(max(first[oy], 0), H - 1);
    const float* w = wt + (long)oy * ksize;
    const float* s = src + (fc * H + j0) * W + x;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < ksize && j0 + k < H; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(s + (long)k * W);
        const float wk = w[k];
        acc.x = fmaf(wk, v.x, acc.x); acc.y = fmaf(wk, v.y, acc.y); acc.z = fmaf(wk, v.z, acc.z); acc.w = fmaf(wk, v.w, acc.w);
    }
    *reinterpret_cast<float4*>(dst + i * 4) = acc;
}

// y pass over interleaved bytes, W % 4 == 0: one thread per four consecutive pixels = 12 bytes = three aligned words per tap
// (a wave reads 768 consecutive bytes of a source row), three 16-byte stores, one per plane
__global__ __launch_bounds__(256) void resample_y4_u8_kernel(const unsigned char* __restrict__ src, int H, int W, const float* __restrict__ wt,
                                                             const int* __restrict__ first, int ksize, int n_out,
                                                             float* __restrict__ dst, long total4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;           // (f, oy, x / 4)
    if (i >= total4) return;
    const int W4 = W >> 2;
    const int x = (int)(i % W4) * 4;
    const long r = i / W4;
    const int oy = (int)(r % n_out);
    const long f = r / n_out;
    const int j0 = min(max(first[oy], 0), H - 1);
    const float* w = wt + (long)oy * ksize;
    const unsigned char* s = src + ((f * H + j0) * W + x) * 3;
    float acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0.f;
    for (int k = 0; k < ksize && j0 + k < H; ++k) {
        const unsigned* p = reinterpret_cast<const unsigned*>(s + (long)k * W * 3);
        const unsigned u[3] = {p[0], p[1], p[2]};
        const float wk = w[k];
#pragma unroll
        for (int e = 0; e < 12; ++e) acc[e] = fmaf(wk, byte_sample((u[e >> 2] >> (8 * (e & 3))) & 0xFFu), acc[e]);   // byte e = pixel e / 3, channel e % 3
    }
    const long plane = (long)n_out * W;
    float* d = dst + (f * 3 * n_out + oy) * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(d + c * plane) = make_float4(acc[c], acc[3 + c], acc[6 + c], acc[9 + c]);
}

// ------------------------------------------------------------------------------------------- patch rows from fp32 planes
// (x - mean) / std as two IEEE operations: no contraction, no reciprocal
__device__ __forceinline__ float normalise(float x, float mean, float std) { return __fdiv_rn(__fsub_rn(x, mean), std); }

// patch % 4 == 0 (so S % 4 == 0 and 3 patch^2 % 4 == 0): one thread per float4 of the output = four consecutive kx of one patch row,
// one 16-byte load and one 16-byte store
__global__ __launch_bounds__(256) void vit_patches_f32x4_kernel(const float* __restrict__ img, int S, int patch, int g,
                                                                const float* __restrict__ mean_std, float* __restrict__ out, int Kp, long total4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int K4 = Kp >> 2;
    const long row = i / K4;
    const int col = (int)(i - row * K4) * 4;
    const int pp = patch * patch;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col < 3 * pp) {
        const int c = col / pp, k = col - c * pp, ky = k / patch, kx = k - ky * patch;
        const long f = row / (g * g);
        const int p = (int)(row - f * g * g), py = p / g, px = p - py * g;
        const float4 x = *reinterpret_cast<const float4*>(img + ((f * 3 + c) * S + py * patch + ky) * S + px * patch + kx);
        const float m = mean_std[c], s = mean_std[3 + c];
        v = make_float4(normalise(x.x, m, s), normalise(x.y, m, s), normalise(x.z, m, s), normalise(x.w, m, s));
    }
    *reinterpret_cast<float4*>(out + i * 4) = v;
}

// any patch size: one thread per output element, as vit_patches_kernel
__global__ __launch_bounds__(256) void vit_patches_f32_kernel(const float* __restrict__ img, int S, int patch, int g,
                                                              const float* __restrict__ mean_std, float* __restrict__ out, int Kp, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long row = i / Kp;
    const int col = (int)(i - row * Kp);
    const int pp = patch * patch;
    float v = 0.f;
    if (col < 3 * pp) {
        const int c = col / pp, k = col - c * pp, ky = k / patch, kx = k - ky * patch;
        const long f = row / (g * g);
        const int p = (int)(row - f * g * g), py = p / g, px = p - py * g;
        v = normalise(img[((f * 3 + c) * S + py * patch + ky) * S + px * patch + kx], mean_std[c], mean_std[3 + c]);
    }
    out[i] = v;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int m324_resample_f32(const void* src, int src_u8, int F, int H, int W, int axis, const float* weights, const int* first,
                                 int ksize, int n_out, float* dst, void* stream) {
    M324_REQUIRE(src && weights && first && dst, "m324_resample_f32: null pointer");
    M324_REQUIRE(F > 0 && H >= 1 && H <= 16384 && W >= 1 && W <= 16384 && n_out >= 1 && n_out <= 16384,
                 "m324_resample_f32: F=%d H=%d W=%d n_out=%d (at least one frame, sides of 1 to 16384)", F, H, W, n_out);
    M324_REQUIRE(axis == 0 || axis == 1, "m324_resample_f32: axis=%d (0 = x, 1 = y)", axis);
    M324_REQUIRE(ksize >= 1 && ksize <= 64, "m324_resample_f32: ksize=%d (1 to 64)", ksize);
    M324_REQUIRE(src_u8 || ((uintptr_t)src & 3) == 0, "m324_resample_f32: an fp32 source must be 4-byte aligned");
    M324_REQUIRE(((uintptr_t)dst & 3) == 0 && ((uintptr_t)weights & 3) == 0 && ((uintptr_t)first & 3) == 0, "m324_resample_f32: misaligned operand");
    const long OH = axis == 0 ? H : n_out, OW = axis == 0 ? n_out : W;
    const long total = (long)F * 3 * OH * OW;
    M324_REQUIRE(total < (1l << 39) && (long)F * 3 * H * W < (1l << 39), "m324_resample_f32: image too large");
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256);
#define RS_GRID(n) dim3((unsigned)(((n) + 255) / 256))
    if (axis == 0 && n_out % 4 == 0 && aligned16(dst)) {
        const long t4 = total / 4;
        if (src_u8) hipLaunchKernelGGL(resample_x4_kernel<true>, RS_GRID(t4), block, 0, s, src, H, W, weights, first, ksize, n_out, dst, t4);
        else hipLaunchKernelGGL(resample_x4_kernel<false>, RS_GRID(t4), block, 0, s, src, H, W, weights, first, ksize, n_out, dst, t4);
    } else if (axis == 1 && W % 4 == 0 && aligned16(dst) && aligned16(src)) {
        if (src_u8) {
            const long t4 = (long)F * n_out * (W / 4);
            hipLaunchKernelGGL(resample_y4_u8_kernel, RS_GRID(t4), block, 0, s, (const unsigned char*)src, H, W, weights, first, ksize, n_out, dst, t4);
        } else {
            const long t4 = total / 4;
            hipLaunchKernelGGL(resample_y4_f32_kernel, RS_GRID(t4), block, 0, s, (const float*)src, H, W, weights, first, ksize, n_out, dst, t4);
        }
    } else {
#define RS_SCALAR(u8, ax) hipLaunchKernelGGL((resample_scalar_kernel<u8, ax>), RS_GRID(total), block, 0, s, src, H, W, weights, first, ksize, n_out, dst, total)
        if (src_u8 && axis == 0) RS_SCALAR(true, 0);
        else if (src_u8) RS_SCALAR(true, 1);
        else if (axis == 0) RS_SCALAR(false, 0);
        else RS_SCALAR(false, 1);
#undef RS_SCALAR
    }
#undef RS_GRID
    M324_CHECK_LAUNCH("m324_resample_f32");
    return M324_OK;
}

extern "C" int m324_vit_patches_f32(const float* img, int F, int S, int patch, const float* mean_std, float* out, int Kp, void* stream) {
    M324_REQUIRE(img && mean_std && out, "m324_vit_patches_f32: null pointer");
    M324_REQUIRE(F > 0 && patch > 0 && S >= patch && S <= 16384 && S % patch == 0, "m324_vit_patches_f32: F=%d S=%d patch=%d (S a multiple of patch, at most 16384)",
                 F, S, patch);
    if (Kp % 32 != 0 || Kp < 3 * patch * patch) M324_FAIL(M324_ERR_UNSUPPORTED, "m324_vit_patches_f32: Kp=%d (Kp %% 32 == 0, at least 3 patch^2 = %d)", Kp, 3 * patch * patch);
    M324_REQUIRE(((uintptr_t)img & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)mean_std & 3) == 0, "m324_vit_patches_f32: misaligned operand");
    const int g = S / patch;
    const long total = (long)F * g * g * Kp;
    M324_REQUIRE(total < (1l << 39), "m324_vit_patches_f32: output too large");
    if (patch % 4 == 0 && aligned16(img) && aligned16(out))
        hipLaunchKernelGGL(vit_patches_f32x4_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, S, patch, g,
                           mean_std, out, Kp, total / 4);
    else
        hipLaunchKernelGGL(vit_patches_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, S, patch, g,
                           mean_std, out, Kp, total);
    M324_CHECK_LAUNCH("m324_vit_patches_f32");
    return M324_OK;
}

extern "C" int m324_attention_tok(const float* qkv, long ld, float* O, long ldo, int B, int L, int H, int D, float scale, void* stream) {
    M324_REQUIRE(qkv && O, "m324_attention_tok: null pointer");
    M324_REQUIRE(B > 0 && H > 0 && L > 0, "m324_attention_tok: empty problem B=%d H=%d L=%d", B, H, L);
    if (D < 8 || D > 128 || D % 8 != 0) M324_FAIL(M324_ERR_UNSUPPORTED, "m324_attention_tok: D=%d (D %% 8 == 0, 8 <= D <= 128)", D);
    M324_REQUIRE(ld >= 3l * H * D && ld % 4 == 0, "m324_attention_tok: ld=%ld (a multiple of 4, at least 3 H D = %ld)", ld, 3l * H * D);
    M324_REQUIRE(ldo >= (long)H * D && ldo % 4 == 0, "m324_attention_tok: ldo=%ld (a multiple of 4, at least H D = %ld)", ldo, (long)H * D);
    M324_REQUIRE(aligned16(qkv) && aligned16(O), "m324_attention_tok: bases must be 16-byte aligned");
    M324_REQUIRE(H <= 65535 && B <= 65535, "m324_attention_tok: grid too large");
    M324_REQUIRE(scale > 0.f && scale < INFINITY, "m324_attention_tok: scale=%g must be positive and finite", (double)scale);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(L, TOK_QB), (unsigned)H, (unsigned)B);
    const float sl2 = scale * 1.4426950408889634f;
    const int DP = (D + 31) / 32 * 32;
#define TOK_LAUNCH(dp, kt) hipLaunchKernelGGL((attn_tok_kernel<dp, kt>), grid, dim3(256), 0, s, qkv, ld, O, ldo, L, H, D, sl2)
    switch (DP) {
        case 32: TOK_LAUNCH(32, 64); break;
        case 64: TOK_LAUNCH(64, 64); break;
        case 96: TOK_LAUNCH(96, 64); break;
        default: TOK_LAUNCH(128, 32); break;
    }
#undef TOK_LAUNCH
    M324_CHECK_LAUNCH("m324_attention_tok");
    return M324_OK;
}

extern "C" int m324_layernorm_wide(const float* x, long ldx, const float* w, const float* b, float eps, float* y, long ldy, int rows,
                                   int C, void* stream) {
    M324_REQUIRE(x && w && y, "m324_layernorm_wide: null pointer");
    M324_REQUIRE(rows > 0, "m324_layernorm_wide: rows=%d", rows);
    if (C < 4 || C > 4096 || C % 4 != 0) M324_FAIL(M324_ERR_UNSUPPORTED, "m324_layernorm_wide: C=%d (C %% 4 == 0, 4 <= C <= 4096)", C);
    M324_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && ldx >= C && ldy >= C, "m324_layernorm_wide: ldx=%ld ldy=%ld (multiples of 4, at least C=%d)",
                 ldx, ldy, C);
    M324_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y) && (!b || aligned16(b)), "m324_layernorm_wide: bases must be 16-byte aligned");
    hipLaunchKernelGGL(layernorm_wide_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, w, b, eps, y,
                       ldy, rows, C);
    M324_CHECK_LAUNCH("m324_layernorm_wide");
    return M324_OK;
}

extern "C" int m324_vit_patches(const unsigned char* img, int F, int S, int patch, const float* mean_std, float* out, int Kp, void* stream) {
    M324_REQUIRE(img && mean_std && out, "m324_vit_patches: null pointer");
    M324_REQUIRE(F > 0 && patch > 0 && S >= patch && S <= 16384 && S % patch == 0, "m324_vit_patches: F=%d S=%d patch=%d (S a multiple of patch, at most 16384)",
                 F, S, patch);
    if (Kp % 32 != 0 || Kp < 3 * patch * patch) M324_FAIL(M324_ERR_UNSUPPORTED, "m324_vit_patches: Kp=%d (Kp %% 32 == 0, at least 3 patch^2 = %d)", Kp, 3 * patch * patch);
    const int g = S / patch;
    const long total = (long)F * g * g * Kp;
    M324_REQUIRE(total < (1l << 39), "m324_vit_patches: output too large");
    hipLaunchKernelGGL(vit_patches_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, S, patch, g, mean_std,
                       out, Kp, total);
    M324_CHECK_LAUNCH("m324_vit_patches");
    return M324_OK;
}

extern "C" int m324_vit_tokens(const float* patch_rows, const float* cls, const float* pos, float* x, int F, int L, int C, void* stream) {
    M324_REQUIRE(patch_rows && cls && pos && x, "m324_vit_tokens: null pointer");
    M324_REQUIRE(F > 0 && L >= 2, "m324_vit_tokens: F=%d L=%d (a class token and at least one patch)", F, L);
    if (C < 4 || C % 4 != 0) M324_FAIL(M324_ERR_UNSUPPORTED, "m324_vit_tokens: C=%d (C %% 4 == 0)", C);
    M324_REQUIRE(aligned16(patch_rows) && aligned16(cls) && aligned16(pos) && aligned16(x), "m324_vit_tokens: bases must be 16-byte aligned");
    const long total = (long)F * L * (C / 4);
    M324_REQUIRE(total < (1l << 39), "m324_vit_tokens: output too large");
    hipLaunchKernelGGL(vit_tokens_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, patch_rows, cls, pos, x, L,
                       C / 4, total);
    M324_CHECK_LAUNCH("m324_vit_tokens");
    return M324_OK;
}
