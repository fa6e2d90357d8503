// The 3D convolution, the 3D max-pool, the head and the input preparation behind the video metric (FVD on an I3D trunk,
// motion324_amd/fvd.py): m324_conv3d, m324_conv3d_tile, m324_maxpool3d, m324_i3d_head and m324_fvd_prepare.  The contract of every
// entry point is in include/m324.h; what is here is how.
//
// The convolution has the structure of csrc/conv.hip, one axis more: an implicit GEMM on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32) with M = the OUTPUT voxels of all samples, N = Cout, K = taps x Cin in (tap, channel) order, the tap
// index running (dt, dh, dw) with dw fastest.  A workgroup of four waves owns a tile of 128 voxels by BN = 128, 64 or 32 output
// channels.  A K step is 16 values: four 16-byte pieces per voxel, each piece four channels of ONE tap (Cin % 4 = 0), fetched from
// the NDHWC activation at (t s_t - p_t + dt, h s_h - p_h + dh, w s_w - p_w + dw) or replaced by zeros when that lies outside the
// volume, the voxel is past M or k is past K.  The pieces go to LDS transposed ([k][voxel]); the weights are stored [k][Cout]
// already and go in as they are, zeros for the columns past Cout of a ragged last tile (Cout % 8 = 0 only).  Two LDS stages, one
// barrier per step, no LDS-DMA, no cross-lane arithmetic, no inline assembly.
//
// The sum over k has conv.hip's two levels: the MFMA's fma chain runs over M324_CONV_RUN consecutive k from 0.0f, then the
// accumulators are added to a second set and cleared.  Every output is the same fixed sequence of operations whatever its voxel's
// place in a tile, in the grid or in the batch, and whatever the tile width; then + bias and max(., 0).  A stride only selects
// which voxels are computed: the chain of output o at stride s is the chain of output s o at stride 1 with the same front padding.
//
// What differs from conv.hip: the tap box (1, 3 or 7 cubed) is a compile-time parameter, so the tap -> (dt, dh, dw) split is a
// division by a constant; the strides and the front padding are arguments; the input and the output are channel SLICES (a base
// pointer and a channel stride each), so the branches of an Inception block read a fused scratch tensor and write into the
// block's concatenated output with no copy.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int BM = 128;
constexpr int BK = M324_CONV_KPAD;
constexpr int RUN_STEPS = M324_CONV_RUN / BK;
constexpr int FILL_WORKGROUPS = 512;    // below this many 128-wide tiles the chip is not full and the narrower tile is taken

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

struct Conv3dGeom {
    int T, H, W;            // input volume
    int To, Ho, Wo;         // output volume: ceil(T / st), ...
    int st, sh, sw;         // strides
    int pt, ph, pw;         // front padding
};

// WN waves along the channels, 4 / WN along the voxels: conv.hip's tile
template <int BOX, int BN, int WN>
__global__ __launch_bounds__(THREADS) void conv3d_kernel(const float* __restrict__ a, long lda, const float* __restrict__ wp,
                                                         const float* __restrict__ bias, float* __restrict__ out, long ldo, long M, Conv3dGeom g,
                                                         int Cin, int Cout, int K, int n_tiles, int relu) {
    constexpr int NP = BM / 64;                     // voxels this thread fetches per step
    constexpr int LDA = BM + 4;                     // 4 * LDA = 16 mod 64: the four pieces of 16 voxels land in 64 different banks
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

    // the NP output voxels this thread fetches for, as the input voxel their tap (0, 0, 0) reads (it may lie in the padding)
    const int kq = tid & 3;
    long vox[NP];
    int ot[NP], oh[NP], ow[NP];
    bool pv[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const long p = m0 + (tid >> 2) + 64 * i;
        pv[i] = p < M;
        long r = pv[i] ? p : 0;
        ow[i] = (int)(r % g.Wo) * g.sw - g.pw;
        r /= g.Wo;
        oh[i] = (int)(r % g.Ho) * g.sh - g.ph;
        r /= g.Ho;
        ot[i] = (int)(r % g.To) * g.st - g.pt;
        const long n = r / g.To;
        vox[i] = ((n * g.T + ot[i]) * g.H + oh[i]) * g.W + ow[i];
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
        const int tap = BOX == 1 ? 0 : k / Cin, c = k - tap * Cin;
        const int dt = tap / (BOX * BOX), dh = (tap / BOX) % BOX, dw = tap % BOX;
        const long off = ((long)dt * g.H + dh) * g.W + dw;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const bool ok = pv[i] && k < K && (unsigned)(ot[i] + dt) < (unsigned)g.T && (unsigned)(oh[i] + dh) < (unsigned)g.H &&
                            (unsigned)(ow[i] + dw) < (unsigned)g.W;
            ra[i] = ok ? *reinterpret_cast<const float4*>(a + (vox[i] + off) * lda + c) : zero4();
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
        if (n >= Cout) continue;                    // the ragged last tile, and nothing outside the slice is written
        const float bv0 = bias[n];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long p = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (p < M) {
                    float v = (tot[i][j][r] + acc[i][j][r]) + bv0;
                    if (relu) v = v > 0.f ? v : 0.f;
                    out[p * ldo + n] = v;
                }
            }
    }
}

__device__ __forceinline__ float4 max4(float4 a, float4 b) {
    return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// one thread per four channels of an output voxel; the window is cut at the volume: padding never enters the maximum
__global__ __launch_bounds__(THREADS) void maxpool3d_kernel(const float4* __restrict__ in, float* __restrict__ out, long ldo, long total, Conv3dGeom g,
                                                            int kt, int kh, int kw, int C4) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    const long p = i / C4;
    long r = p;
    const int w0 = (int)(r % g.Wo) * g.sw - g.pw;
    r /= g.Wo;
    const int h0 = (int)(r % g.Ho) * g.sh - g.ph;
    r /= g.Ho;
    const int t0 = (int)(r % g.To) * g.st - g.pt;
    const long n = r / g.To;
    const int ta = t0 < 0 ? 0 : t0, tb = t0 + kt < g.T ? t0 + kt : g.T;
    const int ha = h0 < 0 ? 0 : h0, hb = h0 + kh < g.H ? h0 + kh : g.H;
    const int wa = w0 < 0 ? 0 : w0, wb = w0 + kw < g.W ? w0 + kw : g.W;
    const float ninf = -__builtin_huge_valf();
    float4 v = make_float4(ninf, ninf, ninf, ninf);
    for (int t = ta; t < tb; ++t)
        for (int h = ha; h < hb; ++h) {
            const float4* s = in + (((n * g.T + t) * g.H + h) * g.W) * C4 + c;
            for (int w = wa; w < wb; ++w) v = max4(v, s[(long)w * C4]);
        }
    *reinterpret_cast<float4*>(out + p * ldo + 4 * c) = v;
}

// head, first half: pooled[n, t, c] = (sum over dt in {0, 1}, h, w, in that order, of x[n, t + dt, h, w, c]) / (2 hw hw)
__global__ __launch_bounds__(THREADS) void head_pool_kernel(const float* __restrict__ x, float* __restrict__ pooled, long total, int T, int hw, int C) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const long r = i / C;
    const int t = (int)(r % (T - 1));
    const long n = r / (T - 1);
    const float* s = x + ((n * T + t) * hw * hw) * C + c;
    float sum = 0.f;
    for (int j = 0; j < 2 * hw * hw; ++j) sum = sum + s[(long)j * C];
    pooled[i] = sum / (float)(2 * hw * hw);
}

// head, second half: out[n, j] = (sum over t, in order, of (logit(n, t, j) + b[j])) / (T - 1); logit = four fma chains over the
// channels c = q mod 4, from 0.0f, combined as (q0 + q1) + (q2 + q3)
__global__ __launch_bounds__(THREADS) void head_logits_kernel(const float* __restrict__ pooled, const float* __restrict__ w, const float* __restrict__ b,
                                                              float* __restrict__ out, int samples, int steps, int C, int classes) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= samples * classes) return;
    const int j = i % classes, n = i / classes;
    const float bj = b[j];
    float sum = 0.f;
    for (int t = 0; t < steps; ++t) {
        const float* p = pooled + ((long)n * steps + t) * C;
        float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
        for (int c = 0; c < C; c += 4) {
            q0 = fmaf(p[c], w[(long)c * classes + j], q0);
            q1 = fmaf(p[c + 1], w[(long)(c + 1) * classes + j], q1);
            q2 = fmaf(p[c + 2], w[(long)(c + 2) * classes + j], q2);
            q3 = fmaf(p[c + 3], w[(long)(c + 3) * classes + j], q3);
        }
        sum = sum + (((q0 + q1) + (q2 + q3)) + bj);
    }
    out[i] = sum / (float)steps;
}

// one axis of the bilinear resize (align_corners = false), the rule of m324_upsample_bilinear
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

template <typename T> __device__ __forceinline__ float unit_of(T v);
template <> __device__ __forceinline__ float unit_of<unsigned char>(unsigned char v) { return (float)v / 255.0f; }
template <> __device__ __forceinline__ float unit_of<float>(float v) { return v; }

// one thread per output pixel: resize [H, W] -> [Hr, Wr], crop [Ho, Wo] at (y0, x0), (v - 0.5) * 2, channel 3 = 0
template <typename T>
__global__ __launch_bounds__(THREADS) void fvd_prepare_kernel(const T* __restrict__ src, float4* __restrict__ dst, long total, int H, int W, int Hr,
                                                              int Wr, int y0, int x0, int Ho, int Wo) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % Wo);
    const long r = i / Wo;
    const int y = (int)(r % Ho);
    const long frame = r / Ho;
    const Lerp ly = lerp_of(y + y0, H, Hr), lx = lerp_of(x + x0, W, Wr);
    const T* s = src + frame * H * W * 3;
    const T* p00 = s + ((long)ly.i0 * W + lx.i0) * 3;
    const T* p01 = s + ((long)ly.i0 * W + lx.i1) * 3;
    const T* p10 = s + ((long)ly.i1 * W + lx.i0) * 3;
    const T* p11 = s + ((long)ly.i1 * W + lx.i1) * 3;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float u = ly.l0 * (lx.l0 * unit_of<T>(p00[c]) + lx.l1 * unit_of<T>(p01[c])) +
                        ly.l1 * (lx.l0 * unit_of<T>(p10[c]) + lx.l1 * unit_of<T>(p11[c]));
        v[c] = (u - 0.5f) * 2.0f;
    }
    dst[i] = make_float4(v[0], v[1], v[2], 0.f);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// tile width from Cout and the output voxel count M: 128 where a 128-wide grid still fills the chip, else 64, and 32 for the
// narrow branches; the last tile of a Cout that is no multiple of the width is ragged
int tile_of(long M, int Cout) {
    if (Cout >= 128 && (M + BM - 1) / BM * ((Cout + 127) / 128) >= FILL_WORKGROUPS) return 128;
    return Cout > 32 ? 64 : 32;
}

// The geometry both the convolution and the pool take: volume, per-axis stride 1 or 2, front padding in 0..k - 1
int geometry(const char* name, int samples, int T, int H, int W, int kt, int kh, int kw, int st, int sh, int sw, int pt, int ph, int pw,
             Conv3dGeom* g, long* M) {
    M324_REQUIRE(samples >= 1 && T >= 1 && H >= 1 && W >= 1, "%s: samples, T, H and W must be at least 1, got %d, %d, %d, %d", name, samples, T, H, W);
    M324_REQUIRE((st == 1 || st == 2) && (sh == 1 || sh == 2) && (sw == 1 || sw == 2), "%s: every stride is 1 or 2, got (%d, %d, %d)", name, st, sh, sw);
    M324_REQUIRE(pt >= 0 && pt < kt && ph >= 0 && ph < kh && pw >= 0 && pw < kw,
                 "%s: the front padding must be in 0..k - 1 per axis, got (%d, %d, %d) for the window (%d, %d, %d)", name, pt, ph, pw, kt, kh, kw);
    M324_REQUIRE((long)samples * T * H * W <= 0x7fffffffL, "%s: samples * T * H * W must stay below 2^31, got %ld", name, (long)samples * T * H * W);
    *g = Conv3dGeom{T, H, W, (T - 1) / st + 1, (H - 1) / sh + 1, (W - 1) / sw + 1, st, sh, sw, pt, ph, pw};
    *M = (long)samples * g->To * g->Ho * g->Wo;
    return M324_OK;
}

template <int BOX>
void launch_conv3d(int width, dim3 grid, hipStream_t st, const float* a, long lda, const float* wp, const float* bias, float* out, long ldo, long M,
                   const Conv3dGeom& g, int Cin, int Cout, int K, int n_tiles, int relu) {
    if (width == 128)
        hipLaunchKernelGGL((conv3d_kernel<BOX, 128, 2>), grid, dim3(THREADS), 0, st, a, lda, wp, bias, out, ldo, M, g, Cin, Cout, K, n_tiles, relu);
    else if (width == 64)
        hipLaunchKernelGGL((conv3d_kernel<BOX, 64, 2>), grid, dim3(THREADS), 0, st, a, lda, wp, bias, out, ldo, M, g, Cin, Cout, K, n_tiles, relu);
    else
        hipLaunchKernelGGL((conv3d_kernel<BOX, 32, 1>), grid, dim3(THREADS), 0, st, a, lda, wp, bias, out, ldo, M, g, Cin, Cout, K, n_tiles, relu);
}

}  // namespace

extern "C" int m324_conv3d_tile(long voxels, int Cout) {
    if (voxels < 1 || Cout < 8 || Cout % 8) return M324_ERR_INVALID;
    return tile_of(voxels, Cout);
}

extern "C" int m324_conv3d(const float* a, long lda, const float* wp, const float* bias, float* out, long ldo, int samples, int T, int H, int W,
                           int Cin, int Cout, int box, int st, int sh, int sw, int pt, int ph, int pw, int relu, int tile, void* stream) {
    M324_REQUIRE(a && wp && bias && out, "m324_conv3d: null a, wp, bias or out");
    M324_REQUIRE(box == 1 || box == 3 || box == 7, "m324_conv3d: the tap box is (1,1,1), (3,3,3) or (7,7,7), got side %d", box);
    Conv3dGeom g;
    long M;
    const int rc = geometry("m324_conv3d", samples, T, H, W, box, box, box, st, sh, sw, pt, ph, pw, &g, &M);
    if (rc != M324_OK) return rc;
    M324_REQUIRE(Cin >= 4 && Cin % 4 == 0 && Cin <= M324_CONV_MAX_CHANNELS, "m324_conv3d: Cin must be a multiple of 4 in 4..%d, got %d",
                 M324_CONV_MAX_CHANNELS, Cin);
    M324_REQUIRE(Cout >= 8 && Cout % 8 == 0 && Cout <= M324_CONV_MAX_CHANNELS, "m324_conv3d: Cout must be a multiple of 8 in 8..%d, got %d",
                 M324_CONV_MAX_CHANNELS, Cout);
    M324_REQUIRE(lda >= Cin && lda % 4 == 0 && lda <= M324_CONV3D_MAX_STRIDE, "m324_conv3d: lda must be a multiple of 4 in Cin..%d, got %ld for Cin %d",
                 M324_CONV3D_MAX_STRIDE, lda, Cin);
    M324_REQUIRE(ldo >= Cout && ldo % 4 == 0 && ldo <= M324_CONV3D_MAX_STRIDE, "m324_conv3d: ldo must be a multiple of 4 in Cout..%d, got %ld for Cout %d",
                 M324_CONV3D_MAX_STRIDE, ldo, Cout);
    M324_REQUIRE(aligned16(a) && aligned16(wp) && aligned16(out), "m324_conv3d: a, wp and out must be 16-byte aligned");
    M324_REQUIRE(((uintptr_t)bias & 3) == 0, "m324_conv3d: bias must be 4-byte aligned");
    M324_REQUIRE(relu == 0 || relu == 1, "m324_conv3d: relu is 0 or 1, got %d", relu);
    M324_REQUIRE(tile == 0 || tile == 32 || tile == 64 || tile == 128, "m324_conv3d: tile is 0 (chosen here), 32, 64 or 128, got %d", tile);
    const int width = tile ? tile : tile_of(M, Cout);
    const int K = box * box * box * Cin;
    const int n_tiles = (Cout + width - 1) / width;
    const long blocks = (M + BM - 1) / BM * n_tiles;
    M324_REQUIRE(blocks <= 0x7fffffffL, "m324_conv3d: %ld workgroups are more than a grid holds", blocks);
    const dim3 grid((unsigned)blocks);
    hipStream_t s = (hipStream_t)stream;
    if (box == 1)
        launch_conv3d<1>(width, grid, s, a, lda, wp, bias, out, ldo, M, g, Cin, Cout, K, n_tiles, relu);
    else if (box == 3)
        launch_conv3d<3>(width, grid, s, a, lda, wp, bias, out, ldo, M, g, Cin, Cout, K, n_tiles, relu);
    else
        launch_conv3d<7>(width, grid, s, a, lda, wp, bias, out, ldo, M, g, Cin, Cout, K, n_tiles, relu);
    M324_CHECK_LAUNCH("m324_conv3d");
    return M324_OK;
}

extern "C" int m324_maxpool3d(const float* in, float* out, long ldo, int samples, int T, int H, int W, int C, int kt, int kh, int kw, int st, int sh,
                              int sw, int pt, int ph, int pw, void* stream) {
    M324_REQUIRE(in && out, "m324_maxpool3d: null in or out");
    M324_REQUIRE((kt == 1 && kh == 3 && kw == 3) || (kt == 3 && kh == 3 && kw == 3) || (kt == 2 && kh == 2 && kw == 2),
                 "m324_maxpool3d: the window is (1,3,3), (3,3,3) or (2,2,2), got (%d, %d, %d)", kt, kh, kw);
    Conv3dGeom g;
    long M;
    const int rc = geometry("m324_maxpool3d", samples, T, H, W, kt, kh, kw, st, sh, sw, pt, ph, pw, &g, &M);
    if (rc != M324_OK) return rc;
    M324_REQUIRE(C >= 4 && C % 4 == 0 && C <= M324_CONV_MAX_CHANNELS, "m324_maxpool3d: C must be a multiple of 4 in 4..%d, got %d", M324_CONV_MAX_CHANNELS, C);
    M324_REQUIRE(ldo >= C && ldo % 4 == 0 && ldo <= M324_CONV3D_MAX_STRIDE, "m324_maxpool3d: ldo must be a multiple of 4 in C..%d, got %ld for C %d",
                 M324_CONV3D_MAX_STRIDE, ldo, C);
    M324_REQUIRE(aligned16(in) && aligned16(out), "m324_maxpool3d: in and out must be 16-byte aligned");
    const long total = M * (C / 4);
    const long blocks = (total + THREADS - 1) / THREADS;
    M324_REQUIRE(blocks <= 0x7fffffffL, "m324_maxpool3d: %ld workgroups are more than a grid holds", blocks);
    hipLaunchKernelGGL(maxpool3d_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, (const float4*)in, out, ldo, total, g, kt, kh,
                       kw, C / 4);
    M324_CHECK_LAUNCH("m324_maxpool3d");
    return M324_OK;
}

extern "C" int m324_i3d_head(const float* x, const float* w, const float* b, float* pooled, float* out, int samples, int T, int hw, int C, int classes,
                             void* stream) {
    M324_REQUIRE(x && w && b && pooled && out, "m324_i3d_head: null x, w, b, pooled or out");
    M324_REQUIRE(samples >= 1 && samples <= M324_I3D_HEAD_MAX_SAMPLES, "m324_i3d_head: samples must be in 1..%d, got %d", M324_I3D_HEAD_MAX_SAMPLES, samples);
    M324_REQUIRE(T >= 2 && T <= M324_I3D_HEAD_MAX_SIDE, "m324_i3d_head: T must be in 2..%d (the window takes two time steps), got %d",
                 M324_I3D_HEAD_MAX_SIDE, T);
    M324_REQUIRE(hw >= 1 && hw <= M324_I3D_HEAD_MAX_SIDE, "m324_i3d_head: hw must be in 1..%d, got %d", M324_I3D_HEAD_MAX_SIDE, hw);
    M324_REQUIRE(C >= 4 && C % 4 == 0 && C <= M324_CONV_MAX_CHANNELS, "m324_i3d_head: C must be a multiple of 4 in 4..%d, got %d", M324_CONV_MAX_CHANNELS, C);
    M324_REQUIRE(classes >= 1 && classes <= M324_CONV_MAX_CHANNELS, "m324_i3d_head: classes must be in 1..%d, got %d", M324_CONV_MAX_CHANNELS, classes);
    M324_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)b | (uintptr_t)pooled | (uintptr_t)out) & 3) == 0, "m324_i3d_head: every pointer must be 4-byte aligned");
    const long total = (long)samples * (T - 1) * C;
    hipLaunchKernelGGL(head_pool_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, x, pooled, total, T, hw, C);
    M324_CHECK_LAUNCH("m324_i3d_head");
    hipLaunchKernelGGL(head_logits_kernel, dim3((unsigned)((samples * classes + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, pooled, w, b,
                       out, samples, T - 1, C, classes);
    M324_CHECK_LAUNCH("m324_i3d_head");
    return M324_OK;
}

extern "C" int m324_fvd_prepare(const void* src, int mode, long frames, int H, int W, int Hr, int Wr, int y0, int x0, int Ho, int Wo, float* dst,
                                void* stream) {
    M324_REQUIRE(src && dst, "m324_fvd_prepare: null src or dst");
    M324_REQUIRE(mode == M324_FVD_U8 || mode == M324_FVD_F32, "m324_fvd_prepare: mode is M324_FVD_U8 or M324_FVD_F32, got %d", mode);
    M324_REQUIRE(frames >= 1 && H >= 1 && W >= 1 && Hr >= 1 && Wr >= 1 && Ho >= 1 && Wo >= 1,
                 "m324_fvd_prepare: frames and all sizes must be at least 1, got %ld, %d x %d -> %d x %d -> %d x %d", frames, H, W, Hr, Wr, Ho, Wo);
    M324_REQUIRE(H <= M324_MATTE_MAX_SIDE && W <= M324_MATTE_MAX_SIDE && Hr <= M324_MATTE_MAX_SIDE && Wr <= M324_MATTE_MAX_SIDE,
                 "m324_fvd_prepare: sizes up to %d, got %d x %d -> %d x %d", M324_MATTE_MAX_SIDE, H, W, Hr, Wr);
    M324_REQUIRE(y0 >= 0 && x0 >= 0 && y0 + Ho <= Hr && x0 + Wo <= Wr, "m324_fvd_prepare: the crop %d x %d at (%d, %d) leaves the resized %d x %d", Ho, Wo,
                 y0, x0, Hr, Wr);
    M324_REQUIRE(frames <= 0x7fffffffL / ((long)H * W) && frames <= 0x7fffffffL / ((long)Ho * Wo),
                 "m324_fvd_prepare: frames * H * W and frames * Ho * Wo must stay below 2^31");
    M324_REQUIRE(aligned16(dst) && (mode == M324_FVD_U8 || ((uintptr_t)src & 3) == 0), "m324_fvd_prepare: dst must be 16-byte, fp32 src 4-byte aligned");
    const long total = frames * Ho * Wo;
    const dim3 grid((unsigned)((total + THREADS - 1) / THREADS));
    if (mode == M324_FVD_U8)
        hipLaunchKernelGGL(fvd_prepare_kernel<unsigned char>, grid, dim3(THREADS), 0, (hipStream_t)stream, (const unsigned char*)src, (float4*)dst, total, H,
                           W, Hr, Wr, y0, x0, Ho, Wo);
    else
        hipLaunchKernelGGL(fvd_prepare_kernel<float>, grid, dim3(THREADS), 0, (hipStream_t)stream, (const float*)src, (float4*)dst, total, H, W, Hr, Wr, y0,
                           x0, Ho, Wo);
    M324_CHECK_LAUNCH("m324_fvd_prepare");
    return M324_OK;
}
