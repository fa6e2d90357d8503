// Block-scaled FP8 ("MX") inference GEMMs: m324_mx_quant, m324_layernorm_mx, m324_gemm_mx.
//
// An MX operand of a [rows, K] matrix is two arrays: q [rows, ldq] e4m3 elements (OCP e4m3fn, one byte each) and
// s [rows, lds] E8M0 scales (one byte per 32 consecutive K of a row, value 2^(byte - 127)).  The quantisation rule, the one
// definition every kernel here and the tests' numpy reference use, for each block of 32 values:
//   X = ceil(log2(amax / 448)) clamped to [-127, 127], scale byte X + 127, elements v * 2^-X rounded to nearest even e4m3
//   (no element saturates: |v| 2^-X <= 448, the largest e4m3 value).  OCP's rule takes floor(log2(amax)) - 8 and clips
//   the values between 448 and 512; this one never clips.
//   An all-zero block: byte 0, zero elements.  A block holding NaN or Inf: byte 0xFF (NaN) and every element 0x7F (NaN),
//   so that the non-finite value reaches the GEMM output rows the way it does in the bf16 kernels.
//
// m324_gemm_mx runs v_mfma_scale_f32_32x32x64_f8f6f4 (cbsz = blgp = e4m3): 2x the bf16 MFMA rate per clock, half the operand
// bytes.  Tile, LDS image and pipeline are m324_gemm's v2 (gemm.hip): 128 x 128 outputs per 4-wave workgroup, LDS rows of 128
// bytes of K -- here 128 e4m3 values, i.e. 4 scale bytes per row and K-tile -- staged by LDS-DMA, double-buffered (tile kt + 1's
// pieces fly under tile kt's MFMAs: alias-scoped LDS views, gemm_mx_body), one barrier per K-tile.  The scales ride with the tiles: each lane loads the scale dwords of its two A rows and two W rows one
// K-tile ahead into registers.
// Operand lane map (32x32x64, e4m3; established with exact integer data, tests/test_mx_kernels_gpu.py): lane l holds row
// l & 31; its registers 0-3 hold k = 16 h .. 16 h + 15 and registers 4-7 k = 32 + 16 h .. + 15 of the 64-k step (h = l >> 5),
// i.e. registers 0-3 of both lane halves are the step's first scale block and registers 4-7 its second.  The scale of the
// first block comes from the lanes of half 0, that of the second from half 1: the scale dword of a row holds the 4 blocks of
// the K-tile, a lane shifts it right by 8 h and the opsel byte 2 ks then picks block 2 ks + h for k-step ks.
// Accumulators are SWAPPED (acc = W . A^T: lane = output row, registers = columns), the layout of gemm_tile.h's
// store_tile_lds, which supplies the bf16 / q|k|v-heads / fp32 residual epilogues unchanged (the C/D layout of the scaled MFMA
// is the bf16 one).  The MX output (fc1 -> fc2) is this file's own epilogue: after the same LDS bounce a row's 64 columns sit in
// 8 lanes of 8 values, a scale block is 4 of those lanes (max by two xor shuffles), and each lane stores 8 element bytes.
#include "gemm_tile.h"

namespace {

constexpr int MX_BLOCK = 32;
typedef int i32x8 __attribute__((ext_vector_type(8)));

// X of the rule above from the bit pattern of a finite, non-zero amax: amax = f 2^E with f in [1, 2) -> the smallest X with
// amax <= 448 2^X = 1.75 2^(8 + X) is E - 8 when f <= 1.75, else E - 7 (exact: no division, no log).
__device__ __forceinline__ int mx_exponent(unsigned abits) {
    int E;
    unsigned mant;
    if (abits >= 0x00800000u) {
        E = (int)(abits >> 23) - 127;
        mant = abits & 0x007FFFFFu;
    } else {                                      // fp32 subnormal: normalise
        const int p = 31 - __builtin_clz(abits);  // abits = 2^p (1 + ...) * 2^-149
        E = p - 149;
        mant = (abits << (23 - p)) & 0x007FFFFFu;
    }
    int X = E - (mant <= 0x00600000u ? 8 : 7);
    return X < -127 ? -127 : (X > 127 ? 127 : X);
}

// Scale byte and the factor 2^-X of a block whose |v| bit patterns have the maximum abits (shared by the block's lanes).
// nonfinite: abits >= 0x7F800000.  Returns the byte; mul receives 2^-X (0 for zero and non-finite blocks).
__device__ __forceinline__ unsigned mx_block_scale(unsigned abits, float& mul) {
    if (abits >= 0x7F800000u) { mul = 0.f; return 0xFFu; }
    if (abits == 0u) { mul = 0.f; return 0u; }
    const int X = mx_exponent(abits);             // finite amax <= 2^128: X <= 120, 2^-X is a normal float
    mul = __uint_as_float((unsigned)(127 - X) << 23);
    return (unsigned)(X + 127);
}

// four values -> four e4m3 bytes (v_cvt_pk_fp8_f32: OCP e4m3fn, round to nearest even); |v mul| <= 448 never saturates.
// A non-finite block (sbyte 0xFF) gets NaN elements, an all-zero block +0 elements.
__device__ __forceinline__ unsigned mx_pack4(float a, float b, float c, float d, float mul, unsigned sbyte) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a * mul, b * mul, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c * mul, d * mul, w, true);
    return sbyte == 0xFFu ? 0x7F7F7F7Fu : (mul == 0.f ? 0u : (unsigned)w);      // zero block: +0 elements (no -0)
}

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }
// max over the aligned group of 4 (8) lanes: xor shuffles inside the group
__device__ __forceinline__ unsigned group4_max(unsigned v) {
    v = umax(v, (unsigned)__shfl_xor((int)v, 1, 64));
    return umax(v, (unsigned)__shfl_xor((int)v, 2, 64));
}
__device__ __forceinline__ unsigned group8_max(unsigned v) {
    v = group4_max(v);
    return umax(v, (unsigned)__shfl_xor((int)v, 4, 64));
}

// ------------------------------------------------------------------------------------------------ m324_mx_quant
// Four lanes per 32-value block, 8 values each: a wave covers 16 blocks = 512 consecutive values of one row.
template <typename TX>
__global__ __launch_bounds__(256) void mx_quant_kernel(const TX* __restrict__ x, long ldx, int rows, int K,
                                                       unsigned char* __restrict__ q, long ldq, unsigned char* __restrict__ s,
                                                       long lds) {
    const int nb = K / MX_BLOCK;
    const long g = (long)blockIdx.x * 64 + (threadIdx.x >> 2);        // block index over rows x nb
    if (g >= (long)rows * nb) return;                                 // the 4 lanes of a block leave together
    const int row = (int)(g / nb), blk = (int)(g - (long)row * nb);
    const int c = blk * MX_BLOCK + (threadIdx.x & 3) * 8;
    float v[8];
    load8(x + (long)row * ldx + c, v);
    unsigned a = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) a = umax(a, abs_bits(v[i]));
    a = group4_max(a);
    float mul;
    const unsigned sb = mx_block_scale(a, mul);
    *reinterpret_cast<uint2*>(q + (long)row * ldq + c) =
        make_uint2(mx_pack4(v[0], v[1], v[2], v[3], mul, sb), mx_pack4(v[4], v[5], v[6], v[7], mul, sb));
    if ((threadIdx.x & 3) == 0) s[(long)row * lds + blk] = (unsigned char)sb;
}

// ------------------------------------------------------------------------------------------------ m324_layernorm_mx
// One wave per row (C <= 1024): pass p, lane l holds columns 256 p + 4 l .. + 3; a scale block is 8 consecutive lanes.
// Two-pass statistics like m324_layernorm (mean, then the sum of squared deviations), y = (x - mean) rstd w + b in fp32, then
// the rule above.
__global__ __launch_bounds__(256) void layernorm_mx_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ w,
                                                           const float* __restrict__ b, float eps, int rows, int C,
                                                           unsigned char* __restrict__ q, long ldq, unsigned char* __restrict__ s,
                                                           long lds) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (long)row * ldx;
    float4 v[4];
    float sum = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int c = p * 256 + lane * 4;
        v[p] = c < C ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        sum += (v[p].x + v[p].y) + (v[p].z + v[p].w);
    }
    const float mean = wave_sum(sum) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if (p * 256 + lane * 4 < C) {
            const float a = v[p].x - mean, bb = v[p].y - mean, cc = v[p].z - mean, d = v[p].w - mean;
            sq += a * a + bb * bb + cc * cc + d * d;
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int c = p * 256 + lane * 4;
        if (p * 256 >= C) break;                                     // wave-uniform
        const bool in = c < C;                                       // C % 32 == 0: a block's 8 lanes are all in or all out
        const int cl = in ? c : 0;
        const float4 ww = *reinterpret_cast<const float4*>(w + cl);
        const float4 bi = b ? *reinterpret_cast<const float4*>(b + cl) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float y0 = (v[p].x - mean) * rstd * ww.x + bi.x, y1 = (v[p].y - mean) * rstd * ww.y + bi.y;
        const float y2 = (v[p].z - mean) * rstd * ww.z + bi.z, y3 = (v[p].w - mean) * rstd * ww.w + bi.w;
        unsigned a = umax(umax(abs_bits(y0), abs_bits(y1)), umax(abs_bits(y2), abs_bits(y3)));
        a = group8_max(a);
        float mul;
        const unsigned sb = mx_block_scale(a, mul);
        if (in) {
            *reinterpret_cast<unsigned*>(q + (long)row * ldq + c) = mx_pack4(y0, y1, y2, y3, mul, sb);
            if ((lane & 7) == 0) s[(long)row * lds + c / MX_BLOCK] = (unsigned char)sb;
        }
    }
}

// ------------------------------------------------------------------------------------------------ m324_gemm_mx
// One K-tile (128 k) of MFMAs for a wave's 64 x 64 block: two k-steps of 64; sa_w / sb_a: the wave's scale dwords of its two W
// rows / two A rows, already shifted by 8 (lane >> 5).
__device__ __forceinline__ void mma_tile_mx(const unsigned char* sa, const unsigned char* sb, int arow0, int brow0, int hi,
                                            const unsigned (&sc_a)[2], const unsigned (&sc_w)[2], f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        i32x8 af[2], wf[2];
        const int c0 = ks * 4 + hi;                      // this lane's k: 16-byte chunks c0 (block 2 ks) and c0 + 2 (block 2 ks + 1)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int4 a0 = *reinterpret_cast<const int4*>(sa + lds_off(arow0 + i * 32, c0));
            const int4 a1 = *reinterpret_cast<const int4*>(sa + lds_off(arow0 + i * 32, c0 + 2));
            const int4 w0 = *reinterpret_cast<const int4*>(sb + lds_off(brow0 + i * 32, c0));
            const int4 w1 = *reinterpret_cast<const int4*>(sb + lds_off(brow0 + i * 32, c0 + 2));
            af[i] = i32x8{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            wf[i] = i32x8{w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = ks == 0
                    ? __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[j], af[i], acc[i][j], 0, 0, 0, (int)sc_w[j], 0, (int)sc_a[i])
                    : __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[j], af[i], acc[i][j], 0, 0, 2, (int)sc_w[j], 2, (int)sc_a[i]);
    }
}

// GELU -> MX epilogue of a wave's 64 x 64 block (swapped accumulators, bounced through the wave's LDS scratch as body8 of
// store_tile_lds does): lane (r8 = lane >> 3, c8 = 8 (lane & 7)) works rows mw + 32 i + 8 p + r8, columns nw + c8 .. + 7.
// N % 64 == 0 (host): a wave's columns are all in or all out.
__device__ __forceinline__ void store_tile_mx(const f32x16 (&acc)[2][2], float* scr, unsigned char* q, long ldq, unsigned char* sq,
                                              long lds, int M, int N, int mw, int nw, int lane, const Epilogue& ep) {
    if (nw >= N) return;
    const int l31 = lane & 31, hi = lane >> 5;
    const int r8 = lane >> 3, c8 = (lane & 7) * 8, n8 = nw + c8;
    float* wr = scr + l31 * EP_LD + 4 * hi;
    const float* rd8 = scr + r8 * EP_LD + c8;
    float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
    if (ep.bias) { b0 = *reinterpret_cast<const float4*>(ep.bias + n8); b1 = *reinterpret_cast<const float4*>(ep.bias + n8 + 4); }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(wr + j * 32 + 8 * g) =
                    make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
        float4 v0[4], v1[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            v0[p] = *reinterpret_cast<const float4*>(rd8 + p * 8 * EP_LD);
            v1[p] = *reinterpret_cast<const float4*>(rd8 + p * 8 * EP_LD + 4);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float4 x = v0[p], y = v1[p];
            x.x += b0.x; x.y += b0.y; x.z += b0.z; x.w += b0.w;
            y.x += b1.x; y.y += b1.y; y.z += b1.z; y.w += b1.w;
            if (ep.act == M324_ACT_GELU) {                // A-S erf (|error| 1.5e-7): the bf16 epilogue's polynomial (6e-5) is
                x.x = gelu_fast(x.x); x.y = gelu_fast(x.y);  // coarser than the e4m3 step of the small values of a block
                x.z = gelu_fast(x.z); x.w = gelu_fast(x.w);
                y.x = gelu_fast(y.x); y.y = gelu_fast(y.y);
                y.z = gelu_fast(y.z); y.w = gelu_fast(y.w);
            }
            unsigned a = umax(umax(umax(abs_bits(x.x), abs_bits(x.y)), umax(abs_bits(x.z), abs_bits(x.w))),
                              umax(umax(abs_bits(y.x), abs_bits(y.y)), umax(abs_bits(y.z), abs_bits(y.w))));
            a = group4_max(a);                           // the 4 lanes of this 32-column block (all lanes take part)
            float mul;
            const unsigned sb = mx_block_scale(a, mul);
            const long m = mw + i * 32 + p * 8 + r8;
            if (m < M) {
                *reinterpret_cast<uint2*>(q + m * ldq + n8) =
                    make_uint2(mx_pack4(x.x, x.y, x.z, x.w, mul, sb), mx_pack4(y.x, y.y, y.z, y.w, mul, sb));
                if ((lane & 3) == 0) sq[m * lds + n8 / MX_BLOCK] = (unsigned char)sb;
            }
        }
    }
}

// OUT: 0 bf16 (bias, or the q|k|v heads: ACT 4), 1 fp32 residual update (bias, gamma, residual = C), 2 MX (bias, GELU)
// The body sees the two stages through THREE __restrict__ views -- LDS-DMA destinations (ring_w), fragment reads (ring_r), epilogue
// scratch -- as the ring kernels of gemm.hip do: otherwise hipcc's wait-count pass takes the fragment reads of tile kt for possible
// readers of the bytes tile kt + 1's DMA is writing and puts `s_waitcnt vmcnt` in front of them, which drains the next tile's
// pieces before the first MFMA of the current one (no load / compute overlap at all).  INVARIANT the views rest on: every conflicting
// pair -- a stage's fill and its reads, its last read and its refill, the last reads and the epilogue's scratch -- is separated by a
// counted vmcnt wait AND the workgroup barrier, both in one `asm volatile(... ::: "memory")` that no LLVM pass moves memory
// operations across.  tests/test_mx_host.py checks the compiled loop: no vmcnt wait between a tile's DMA issue and its MFMAs.
template <int OUT, int ACT>
__device__ __forceinline__ void gemm_mx_body(unsigned char* __restrict__ ring_w, const unsigned char* __restrict__ ring_r,
                                             float* __restrict__ scratch, const unsigned char* __restrict__ A, long lda,
                                             const unsigned char* __restrict__ sA, long ldsa, const unsigned char* __restrict__ W,
                                             long ldw, const unsigned char* __restrict__ sW, long ldsw, void* C, long ldc,
                                             unsigned char* sC, long ldsc, int M, int N, int K, const Epilogue& ep, int ntn,
                                             int xcd_remap) {
    constexpr int BK = ROWB;                                   // 128 e4m3 values of K per LDS row

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, hi = lane >> 5;
    int tm, tn;
    tile_of(blockIdx.x, gridDim.x, (M + BM - 1) / BM, ntn, xcd_remap, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    unsigned va[4], vb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave * 4 + i) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        va[i] = (unsigned)((long)min(r, M - 1 - m0) * lda + c * 16);
        vb[i] = (unsigned)((long)min(r, N - 1 - n0) * ldw + c * 16);
    }
    const __amdgpu_buffer_rsrc_t ra = dma_rsrc(A + (long)m0 * lda), rb = dma_rsrc(W + (long)n0 * ldw);
    auto issue_tile = [&](int kt, int buf) {
        unsigned char* sa = ring_w + buf * 2 * TILE_BYTES + wave * 4096;
        unsigned char* sb = sa + TILE_BYTES;
        const unsigned so = (unsigned)(kt * BK);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dma_piece(ra, sa + i * 1024, va[i], so);
            dma_piece(rb, sb + i * 1024, vb[i], so);
        }
    };
    // scale dwords: rows arow0 + 32 i of A, brow0 + 32 j of W (clamped like the tiles), 4 blocks = one K-tile per dword
    const int arow0 = wm * 64 + l31, brow0 = wn * 64 + l31;
    const unsigned* pa[2];
    const unsigned* pw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        pa[i] = reinterpret_cast<const unsigned*>(sA + (long)min(m0 + arow0 + i * 32, M - 1) * ldsa);
        pw[i] = reinterpret_cast<const unsigned*>(sW + (long)min(n0 + brow0 + i * 32, N - 1) * ldsw);
    }
    const unsigned shift = 8u * (unsigned)hi;
    unsigned sc_a[2], sc_w[2], nx_a[2], nx_w[2];

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = K / BK;
#pragma unroll
    for (int i = 0; i < 2; ++i) { nx_a[i] = pa[i][0]; nx_w[i] = pw[i][0]; }
    issue_tile(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        // tile kt and its scales landed (every wave's pieces: the barrier), and every wave is done reading tile kt - 1's stage,
        // which tile kt + 1 refills below
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
        for (int i = 0; i < 2; ++i) { sc_a[i] = nx_a[i] >> shift; sc_w[i] = nx_w[i] >> shift; }
        if (kt + 1 < nk) {
            issue_tile(kt + 1, (kt + 1) & 1);
#pragma unroll
            for (int i = 0; i < 2; ++i) { nx_a[i] = pa[i][kt + 1]; nx_w[i] = pw[i][kt + 1]; }
        }
        const unsigned char* sa = ring_r + (kt & 1) * 2 * TILE_BYTES;
        mma_tile_mx(sa, sa + TILE_BYTES, arow0, brow0, hi, sc_a, sc_w, acc);
    }
    // all waves are done reading the stages (and nothing is in flight): reuse them as epilogue scratch
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    float* scr = scratch + wave * EP_WAVE_FLOATS;
    if constexpr (OUT == 0)
        store_tile_lds<bf16_t, ACT, 0, 2>(acc, scr, static_cast<bf16_t*>(C), ldc, M, N, m0 + wm * 64, n0 + wn * 64, lane, ep);
    else if constexpr (OUT == 1)
        store_tile_lds<float, 0, 1, 2>(acc, scr, static_cast<float*>(C), ldc, M, N, m0 + wm * 64, n0 + wn * 64, lane, ep);
    else
        store_tile_mx(acc, scr, static_cast<unsigned char*>(C), ldc, sC, ldsc, M, N, m0 + wm * 64, n0 + wn * 64, lane, ep);
}

template <int OUT, int ACT>
__global__ __launch_bounds__(256, 2) void gemm_mx_kernel(const unsigned char* __restrict__ A, long lda, const unsigned char* __restrict__ sA,
                                                         long ldsa, const unsigned char* __restrict__ W, long ldw,
                                                         const unsigned char* __restrict__ sW, long ldsw, void* C, long ldc,
                                                         unsigned char* sC, long ldsc, int M, int N, int K, Epilogue ep, int ntn,
                                                         int xcd_remap) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[4 * TILE_BYTES];   // A0 B0 A1 B1
    gemm_mx_body<OUT, ACT>(smem, smem, reinterpret_cast<float*>(smem), A, lda, sA, ldsa, W, ldw, sW, ldsw, C, ldc, sC, ldsc, M, N, K,
                           ep, ntn, xcd_remap);
}

bool al(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

}  // namespace

extern "C" int m324_mx_quant(const void* x, int x_dtype, long ldx, int rows, int K, void* q, long ldq, void* s, long lds,
                             void* stream) {
    M324_REQUIRE(x && q && s, "m324_mx_quant: null pointer");
    M324_REQUIRE(x_dtype == M324_F32 || x_dtype == M324_BF16, "m324_mx_quant: x_dtype %d (fp32 or bf16)", x_dtype);
    M324_REQUIRE(rows > 0 && K > 0 && K % MX_BLOCK == 0, "m324_mx_quant: rows=%d K=%d (K %% 32 == 0)", rows, K);
    M324_REQUIRE(ldx >= K && ldq >= K && lds >= K / MX_BLOCK, "m324_mx_quant: leading dimension too small");
    const int esz = x_dtype == M324_F32 ? 4 : 2;
    M324_REQUIRE(al(x, 16) && (ldx * esz) % 16 == 0 && al(q, 8) && ldq % 8 == 0, "m324_mx_quant: x rows must be 16-byte, q rows 8-byte aligned");
    const long blocks = (long)rows * (K / MX_BLOCK);
    const int grid = ceil_div(blocks, 64);
    if (x_dtype == M324_F32)
        hipLaunchKernelGGL(mx_quant_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx, rows, K,
                           (unsigned char*)q, ldq, (unsigned char*)s, lds);
    else
        hipLaunchKernelGGL(mx_quant_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, rows, K,
                           (unsigned char*)q, ldq, (unsigned char*)s, lds);
    M324_CHECK_LAUNCH("m324_mx_quant");
    return M324_OK;
}

extern "C" int m324_layernorm_mx(const float* x, long ldx, const float* w, const float* b, float eps, int rows, int C, void* q,
                                 long ldq, void* s, long lds, void* stream) {
    M324_REQUIRE(x && w && q && s, "m324_layernorm_mx: null pointer");
    M324_REQUIRE(rows > 0 && C > 0 && C % MX_BLOCK == 0 && C <= 1024, "m324_layernorm_mx: rows=%d C=%d (C %% 32 == 0, C <= 1024)", rows, C);
    M324_REQUIRE(ldx >= C && ldq >= C && lds >= C / MX_BLOCK, "m324_layernorm_mx: leading dimension too small");
    M324_REQUIRE(al(x, 16) && ldx % 4 == 0 && al(w, 16) && (!b || al(b, 16)) && al(q, 4) && ldq % 4 == 0,
                 "m324_layernorm_mx: x / w / b must be 16-byte, q rows 4-byte aligned");
    hipLaunchKernelGGL(layernorm_mx_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, w, b, eps, rows, C,
                       (unsigned char*)q, ldq, (unsigned char*)s, lds);
    M324_CHECK_LAUNCH("m324_layernorm_mx");
    return M324_OK;
}

extern "C" int m324_gemm_mx(const m324_gemm_args* a, const void* A_scale, long lds_a, const void* W_scale, long lds_w, void* C_scale,
                            long lds_c, void* stream) {
    M324_REQUIRE(a, "m324_gemm_mx: null arguments");
    const bool qkv = a->aux_mode == M324_AUX_QKV_HEADS || a->aux_mode == M324_AUX_QKV_HEADS_VT;
    M324_REQUIRE(a->A && a->W && A_scale && W_scale && (a->C || qkv), "m324_gemm_mx: null pointer");
    M324_REQUIRE(a->in_dtype == M324_MXFP8, "m324_gemm_mx: in_dtype %d (M324_MXFP8 operands only)", a->in_dtype);
    M324_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, "m324_gemm_mx: empty problem M=%d N=%d K=%d", a->M, a->N, a->K);
    if (a->K % 128 != 0) M324_FAIL(M324_ERR_UNSUPPORTED, "m324_gemm_mx: K=%d must be a multiple of 128", a->K);
    if (a->N % 64 != 0) M324_FAIL(M324_ERR_UNSUPPORTED, "m324_gemm_mx: N=%d must be a multiple of 64", a->N);
    if (a->batch > 1) M324_FAIL(M324_ERR_UNSUPPORTED, "m324_gemm_mx: batch=%d (single problems only)", a->batch);
    M324_REQUIRE(a->lda >= a->K && a->ldw >= a->K && lds_a >= a->K / MX_BLOCK && lds_w >= a->K / MX_BLOCK,
                 "m324_gemm_mx: leading dimension too small");
    M324_REQUIRE(al(a->A, 16) && al(a->W, 16) && a->lda % 16 == 0 && a->ldw % 16 == 0 && al(A_scale, 4) && al(W_scale, 4) &&
                 lds_a % 4 == 0 && lds_w % 4 == 0, "m324_gemm_mx: operand rows must be 16-byte, scale rows 4-byte aligned");
    M324_REQUIRE(129l * (a->lda > a->ldw ? a->lda : a->ldw) + a->K < 0x7FFFFFFFl, "m324_gemm_mx: operand tile exceeds the 32-bit DMA offset");
    M324_REQUIRE(!a->bias || al(a->bias, 16), "m324_gemm_mx: bias misaligned");
    // the built epilogues: everything else is refused before anything is launched
    if (a->row_gin > 0 || a->ln_rowstat || a->ln_stats_out || a->ln_copy_out || (a->res_rows > 0 && a->res_rows < a->M))
        M324_FAIL(M324_ERR_UNSUPPORTED, "m324_gemm_mx: no row map, LayerNorm fold or broadcast residual");
    int out = -1, act = 0;
    if (a->out_dtype == M324_BF16 && qkv) {
        M324_REQUIRE(a->act == M324_ACT_NONE && !a->residual && !a->gamma && a->qkv_L > 0 && a->qkv_H > 0 && a->M % a->qkv_L == 0,
                     "m324_gemm_mx: q|k|v heads: no activation / residual / gamma, M a multiple of qkv_L");
        const int parts = (a->qkv_q ? 1 : 0) + (a->qkv_k ? 1 : 0) + (a->qkv_v ? 1 : 0);
        M324_REQUIRE(parts > 0 && a->N == parts * a->qkv_H * 64 && (a->qkv_q || !a->qkv_qw) && (a->qkv_k || !a->qkv_kw),
                     "m324_gemm_mx: q|k|v heads: N=%d vs %d parts of %d heads", a->N, parts, a->qkv_H);
        M324_REQUIRE(a->aux_mode != M324_AUX_QKV_HEADS_VT || (a->qkv_v && a->qkv_L % 128 == 0),
                     "m324_gemm_mx: M324_AUX_QKV_HEADS_VT needs a V output and qkv_L %% 128 == 0");
        M324_REQUIRE(al(a->qkv_q, 16) && al(a->qkv_k, 16) && al(a->qkv_v, 16) && (!a->qkv_qw || al(a->qkv_qw, 16)) &&
                     (!a->qkv_kw || al(a->qkv_kw, 16)), "m324_gemm_mx: q|k|v outputs misaligned");
        out = 0, act = 4;
    } else if (a->aux_mode != M324_AUX_NONE) {
        M324_FAIL(M324_ERR_UNSUPPORTED, "m324_gemm_mx: aux_mode %d", a->aux_mode);
    } else if (a->out_dtype == M324_BF16 && a->act == M324_ACT_NONE && !a->residual && !a->gamma) {
        M324_REQUIRE(a->ldc >= a->N && a->ldc % 8 == 0 && al(a->C, 16), "m324_gemm_mx: bf16 C misaligned / ldc too small");
        out = 0;
    } else if (a->out_dtype == M324_F32 && a->act == M324_ACT_NONE && a->residual && (const void*)a->residual == a->C) {
        M324_REQUIRE(a->ldc >= a->N && a->ldr == a->ldc && a->ldc % 4 == 0 && al(a->C, 16) && (!a->gamma || al(a->gamma, 16)),
                     "m324_gemm_mx: fp32 residual update misaligned");
        out = 1;
    } else if (a->out_dtype == M324_MXFP8 && !a->residual && !a->gamma) {
        M324_REQUIRE(C_scale && a->ldc >= a->N && a->ldc % 8 == 0 && al(a->C, 8) && lds_c >= a->N / MX_BLOCK,
                     "m324_gemm_mx: MX output misaligned / leading dimension too small");
        out = 2;
    }
    if (out < 0)
        M324_FAIL(M324_ERR_UNSUPPORTED, "m324_gemm_mx: epilogue (out_dtype %d, act %d, residual %s, gamma %s) is not built", a->out_dtype,
                  a->act, a->residual ? "yes" : "no", a->gamma ? "yes" : "no");

    const Epilogue ep{a->bias, a->gamma, a->residual, a->ldr, 0, a->act, 0, 0, 0, 0, 0, 0, nullptr, 0, a->aux_mode,
                      {(bf16_t*)a->qkv_q, (bf16_t*)a->qkv_k, (bf16_t*)a->qkv_v}, {a->qkv_qw, a->qkv_kw}, a->qkv_eps, a->qkv_qscale,
                      a->qkv_L, a->qkv_H, a->aux_mode == M324_AUX_QKV_HEADS_VT ? 1 : 0, 0, 0,
                      nullptr, nullptr, nullptr, nullptr, 0, 0, 0.f};
    const int ntm = ceil_div(a->M, BM), ntn = ceil_div(a->N, BN);
    const int xcd = m324::tunable(m324::TUN_XCD) & 1;
    const dim3 grid(ntm * ntn), block(256);
    const hipStream_t s = (hipStream_t)stream;
    const auto* A = (const unsigned char*)a->A;
    const auto* W = (const unsigned char*)a->W;
    const auto* sA = (const unsigned char*)A_scale;
    const auto* sW = (const unsigned char*)W_scale;
    if (out == 0 && act == 4)
        hipLaunchKernelGGL((gemm_mx_kernel<0, 4>), grid, block, 0, s, A, a->lda, sA, lds_a, W, a->ldw, sW, lds_w, a->C, a->ldc,
                           nullptr, 0, a->M, a->N, a->K, ep, ntn, xcd);
    else if (out == 0)
        hipLaunchKernelGGL((gemm_mx_kernel<0, 0>), grid, block, 0, s, A, a->lda, sA, lds_a, W, a->ldw, sW, lds_w, a->C, a->ldc,
                           nullptr, 0, a->M, a->N, a->K, ep, ntn, xcd);
    else if (out == 1)
        hipLaunchKernelGGL((gemm_mx_kernel<1, 0>), grid, block, 0, s, A, a->lda, sA, lds_a, W, a->ldw, sW, lds_w, a->C, a->ldc,
                           nullptr, 0, a->M, a->N, a->K, ep, ntn, xcd);
    else
        hipLaunchKernelGGL((gemm_mx_kernel<2, 0>), grid, block, 0, s, A, a->lda, sA, lds_a, W, a->ldw, sW, lds_w, a->C, a->ldc,
                           (unsigned char*)C_scale, lds_c, a->M, a->N, a->K, ep, ntn, xcd);
    M324_CHECK_LAUNCH("m324_gemm_mx");
    return M324_OK;
}
