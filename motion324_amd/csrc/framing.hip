// Video framing kernels (gfx950): the matte's threshold or soft masking, one bounding box per frame, and the two separable
// passes of Pillow's 8-bit Lanczos resampling that crop a video to the union box and paste it centred on a square canvas -- the
// device twin of utils/rmbg_for_black_bg.py (compute_mask_bbox, merge_bbox, crop_and_center_to_512 and the masking around them;
// a PIL loop per frame in the reference).  motion324_amd/framing.py drives them and builds the coefficient tables on the host.
//
// The arithmetic IS the contract and it is all integer: a mask is a comparison or a table lookup, a box is min / max, a
// resampled byte is clamp((2^21 + sum value * coef) >> 22) in 32-bit two's complement.  Nothing depends on the grid, on the
// order of the atomics or on how much of a span a workgroup could stage.
#include "common.h"
#include <limits.h>
#include <math.h>
#include <algorithm>

namespace {

typedef unsigned char u8;

// ------------------------------------------------------------------------------------------------ masking and boxes
constexpr int MASK_THREADS = 256;
constexpr int MASK_GROUP = 16;                           // pixels per lane: 64 bytes of RGBA, 48 of RGB, 16 of alpha

__global__ __launch_bounds__(MASK_THREADS) void frame_box_init_kernel(int* __restrict__ boxes, int frames, int width, int height) {
    const int t = blockIdx.x * MASK_THREADS + threadIdx.x;
    if (t >= frames) return;
    boxes[4 * t] = width;
    boxes[4 * t + 1] = height;
    boxes[4 * t + 2] = 0;
    boxes[4 * t + 3] = 0;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[12], int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu; }

// One lane = 16 consecutive pixels of one row; one workgroup = 256 such groups of ONE frame (a flat grid, blocks_per_frame
// workgroups per frame).  A pixel travels as r | g << 8 | b << 16 | alpha << 24.
template <bool SOFT>
__global__ __launch_bounds__(MASK_THREADS) void frame_mask_kernel(const u8* __restrict__ src, long src_frame, long src_pitch, int src_pixel,
                                                                  const u8* __restrict__ alpha, long alpha_frame, long alpha_pitch, int alpha_pixel,
                                                                  int height, int width, int groups, int blocks_per_frame, int threshold,
                                                                  const u8* __restrict__ table, u8* __restrict__ masked, u8* __restrict__ mask,
                                                                  int* __restrict__ boxes) {
    __shared__ int part[MASK_THREADS / 64][4];
    const int t = blockIdx.x / blocks_per_frame;
    const long item = (long)(blockIdx.x % blocks_per_frame) * MASK_THREADS + threadIdx.x;
    int min_x = INT_MAX, min_y = INT_MAX, max_x = 0, max_y = 0;          // max_* hold the open end: 0 = nothing seen
    if (item < (long)height * groups) {
        const int y = (int)(item / groups);
        const int x0 = (int)(item % groups) * MASK_GROUP;
        const int n = min(MASK_GROUP, width - x0);
        const u8* p = src + (long)t * src_frame + (long)y * src_pitch + (long)x0 * src_pixel;
        const u8* a = alpha + (long)t * alpha_frame + (long)y * alpha_pitch + (long)x0 * alpha_pixel;
        uint32_t px[MASK_GROUP];
        if (n == MASK_GROUP && src_pixel == 4 && alpha_pixel == 4 && a == p + 3 && aligned16(p)) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 v = reinterpret_cast<const uint4*>(p)[q];
                px[4 * q] = v.x; px[4 * q + 1] = v.y; px[4 * q + 2] = v.z; px[4 * q + 3] = v.w;
            }
        } else if (n == MASK_GROUP && src_pixel == 3 && alpha_pixel == 1 && aligned16(p) && aligned16(a)) {
            uint32_t w[12], aw[4];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = reinterpret_cast<const uint4*>(p)[q];
                w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
            }
            const uint4 av = *reinterpret_cast<const uint4*>(a);
            aw[0] = av.x; aw[1] = av.y; aw[2] = av.z; aw[3] = av.w;
#pragma unroll
            for (int i = 0; i < MASK_GROUP; ++i)
                px[i] = byte_of(w, 3 * i) | (byte_of(w, 3 * i + 1) << 8) | (byte_of(w, 3 * i + 2) << 16) |
                        (((aw[i >> 2] >> ((i & 3) * 8)) & 0xFFu) << 24);
        } else {
#pragma unroll
            for (int i = 0; i < MASK_GROUP; ++i) {
                px[i] = 0;
                if (i < n) {
                    const u8* s = p + (long)i * src_pixel;
                    px[i] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)a[(long)i * alpha_pixel] << 24);
                }
            }
        }
        uint32_t m_bits = 0;                                             // bit i: pixel i of the group is foreground
        uint32_t out_w[12], mask_w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 12; ++q) out_w[q] = 0;
#pragma unroll
        for (int i = 0; i < MASK_GROUP; ++i) {
            const uint32_t al = px[i] >> 24;
            uint32_t m, rgb;
            if (SOFT) {
                m = al;
                const u8* row = table + al * 256u;
                rgb = (uint32_t)row[px[i] & 0xFFu] | ((uint32_t)row[(px[i] >> 8) & 0xFFu] << 8) | ((uint32_t)row[(px[i] >> 16) & 0xFFu] << 16);
            } else {
                m = (int)al > threshold ? 255u : 0u;
                rgb = m ? (px[i] & 0xFFFFFFu) : 0u;
            }
            if (i >= n) { m = 0; rgb = 0; }
            if (m) m_bits |= 1u << i;
            mask_w[i >> 2] |= m << ((i & 3) * 8);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = 3 * i + c;
                out_w[k >> 2] |= ((rgb >> (8 * c)) & 0xFFu) << ((k & 3) * 8);
            }
        }
        if (m_bits) {
            min_x = x0 + (__ffs(m_bits) - 1);
            max_x = x0 + (32 - __clz(m_bits));
            min_y = y;
            max_y = y + 1;
        }
        if (masked) {
            u8* o = masked + (((long)t * height + y) * width + x0) * 3;
            if (n == MASK_GROUP && aligned16(o)) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    reinterpret_cast<uint4*>(o)[q] = make_uint4(out_w[4 * q], out_w[4 * q + 1], out_w[4 * q + 2], out_w[4 * q + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < 3 * MASK_GROUP; ++k)
                    if (k < 3 * n) o[k] = (u8)byte_of(out_w, k);
            }
        }
        if (mask) {
            u8* o = mask + ((long)t * height + y) * width + x0;
            if (n == MASK_GROUP && aligned16(o)) {
                *reinterpret_cast<uint4*>(o) = make_uint4(mask_w[0], mask_w[1], mask_w[2], mask_w[3]);
            } else {
#pragma unroll
                for (int i = 0; i < MASK_GROUP; ++i)
                    if (i < n) o[i] = (u8)((mask_w[i >> 2] >> ((i & 3) * 8)) & 0xFFu);
            }
        }
    }
    // wave, then workgroup, then one atomic per bound and workgroup: min and max commute, so the order never shows
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        min_x = min(min_x, __shfl_xor(min_x, d, 64));
        min_y = min(min_y, __shfl_xor(min_y, d, 64));
        max_x = max(max_x, __shfl_xor(max_x, d, 64));
        max_y = max(max_y, __shfl_xor(max_y, d, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = min_x; part[wave][1] = min_y; part[wave][2] = max_x; part[wave][3] = max_y;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < MASK_THREADS / 64; ++w) {
            min_x = min(min_x, part[w][0]); min_y = min(min_y, part[w][1]);
            max_x = max(max_x, part[w][2]); max_y = max(max_y, part[w][3]);
        }
        if (max_x > 0) {
            atomicMin(boxes + 4 * t, min_x);
            atomicMin(boxes + 4 * t + 1, min_y);
            atomicMax(boxes + 4 * t + 2, max_x);
            atomicMax(boxes + 4 * t + 3, max_y);
        }
    }
}

// ------------------------------------------------------------------------------------------------ one resampling pass
constexpr int RS_THREADS = 256;
constexpr int RS_LDS_BYTES = 48 * 1024;                  // one source line of M324_FRAME_MAX_SIDE pixels x 3 channels
static_assert(M324_FRAME_MAX_SIDE * 3 <= RS_LDS_BYTES, "a whole line must fit");

// A pass seen without its direction: `lines` independent lines of in_size positions; output o of a line is a weighted sum of the
// positions bounds[o][0] .. + bounds[o][1] of the same line.  Strides in bytes; the pointers already include the crop origin.
// The destination is addressed in CANVAS coordinates (line cl, output co); the pass's own result sits at (off_line, off_out) and
// the kernel writes the canvas range [c0, c1) of both, `fill` outside the result.
struct PassArgs {
    const u8* src; long src_frame, src_line, src_pos;
    const u8* alpha; long alpha_frame, alpha_line, alpha_pos;
    const u8* table;
    const int* coef; const int* bounds;
    u8* dst; long dst_frame, dst_line, dst_pos;
    int mode, threshold, in_size, out_size, ksize, lines;
    int off_line, off_out, c0_line, c1_line, c0_out, c1_out, fill;
    int tile_lines, tile_out, tiles_lines, tiles_out, lds_pixels;
    int coef_offset;                                     // byte offset of the staged coefficient rows in LDS, or -1: read from memory
};

// the masked value of one source sample: C channels packed into the low bytes
template <int C>
__device__ __forceinline__ uint32_t fetch(const PassArgs& a, const u8* __restrict__ s, const u8* __restrict__ al) {
    uint32_t v, alpha_v = 0;
    if (C == 3 && al == s + 3 && ((uintptr_t)s & 3) == 0) {              // RGBA, aligned: one load brings the pixel and its alpha
        const uint32_t w = *reinterpret_cast<const uint32_t*>(s);
        v = w & 0xFFFFFFu;
        alpha_v = w >> 24;
    } else {
        v = s[0];
        if (C == 3) v |= ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
        if (a.mode != M324_FRAME_NONE) alpha_v = *al;
    }
    switch (a.mode) {
        case M324_FRAME_THRESHOLD: return (int)alpha_v > a.threshold ? v : 0u;
        case M324_FRAME_BINARY: return (int)alpha_v > a.threshold ? (C == 3 ? 0xFFFFFFu : 0xFFu) : 0u;
        case M324_FRAME_SOFT: {
            const u8* row = a.table + alpha_v * 256u;
            uint32_t r = row[v & 0xFFu];
            if (C == 3) r |= ((uint32_t)row[(v >> 8) & 0xFFu] << 8) | ((uint32_t)row[(v >> 16) & 0xFFu] << 16);
            return r;
        }
        default: return v;
    }
}

// acc[c] += sample * coefficient over n staged taps, `step` bytes apart; inlined, so the coefficient pointer keeps its address space
template <int C>
__device__ __forceinline__ void taps(uint32_t (&acc)[C], const u8* __restrict__ s, int step, const int* __restrict__ k, int n) {
#pragma unroll 4
    for (int q = 0; q < n; ++q) {
        const uint32_t w = (uint32_t)k[q];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += (uint32_t)s[c] * w;
        s += step;
    }
}

// One workgroup = (frame, tile of lines, tile of outputs).  LINES_INNER: neighbouring lanes take neighbouring LINES (the pass
// along y, whose lines are the bytes of a row: coalesced reads and writes); otherwise neighbouring outputs of one line (the pass
// along x).  The span of source positions the tile's outputs read is staged once, masked, C bytes per sample; a tap outside
// what fitted (or outside what a foreign table promised) is fetched from memory instead, with the same result.  Along x every
// lane walks a coefficient row of its own, ksize ints apart in memory (one cache line per lane and tap); the tile's rows are
// therefore staged too, with contiguous loads, and read back at a stride of ksize words -- odd, so free of bank conflicts.
template <int C, bool LINES_INNER>
__global__ __launch_bounds__(RS_THREADS) void frame_resample_kernel(const PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) u8 staged_px[];
    __shared__ int span[2];
    const int tid = threadIdx.x;
    const int to = blockIdx.x % a.tiles_out;
    const int tl = (blockIdx.x / a.tiles_out) % a.tiles_lines;
    const int t = blockIdx.x / (a.tiles_out * a.tiles_lines);
    const int cl0 = a.c0_line + tl * a.tile_lines, co0 = a.c0_out + to * a.tile_out;
    const int ncl = min(a.tile_lines, a.c1_line - cl0), nco = min(a.tile_out, a.c1_out - co0);
    // the part of the tile that lies inside the pass's result
    const int l_lo = max(cl0 - a.off_line, 0), l_hi = min(cl0 + ncl - a.off_line, a.lines);
    const int o_lo = max(co0 - a.off_out, 0), o_hi = min(co0 + nco - a.off_out, a.out_size);
    const bool any = l_lo < l_hi && o_lo < o_hi;
    const int nl = any ? l_hi - l_lo : 0;

    if (tid == 0) { span[0] = a.in_size; span[1] = 0; }
    __syncthreads();
    if (any) {
        int lo = a.in_size, hi = 0;
        for (int o = o_lo + tid; o < o_hi; o += RS_THREADS) {
            const int x = min(max(a.bounds[2 * o], 0), a.in_size);
            const int n = min(max(a.bounds[2 * o + 1], 0), min(a.ksize, a.in_size - x));
            if (n > 0) { lo = min(lo, x); hi = max(hi, x + n); }
        }
        if (lo < hi) { atomicMin(&span[0], lo); atomicMax(&span[1], hi); }
    }
    __syncthreads();
    const int s_lo = span[0];
    const int n_staged = any && span[1] > s_lo ? min(span[1] - s_lo, a.lds_pixels / nl) : 0;

    const u8* src_t = a.src + (long)t * a.src_frame;
    const u8* alpha_t = a.alpha ? a.alpha + (long)t * a.alpha_frame : nullptr;
    const int total = n_staged * nl;
    for (int idx = tid; idx < total; idx += RS_THREADS) {
        const int l = LINES_INNER ? idx % nl : idx / n_staged;
        const int p = LINES_INNER ? idx / nl : idx % n_staged;
        const u8* s = src_t + (long)(l_lo + l) * a.src_line + (long)(s_lo + p) * a.src_pos;
        const u8* al = alpha_t ? alpha_t + (long)(l_lo + l) * a.alpha_line + (long)(s_lo + p) * a.alpha_pos : nullptr;
        const uint32_t v = fetch<C>(a, s, al);
#pragma unroll
        for (int c = 0; c < C; ++c) staged_px[idx * C + c] = (u8)(v >> (8 * c));
    }
    const bool coef_staged = !LINES_INNER && a.coef_offset >= 0;        // row o is then at staged_coef + (o - o_lo) * ksize
    int* staged_coef = reinterpret_cast<int*>(staged_px + (coef_staged ? a.coef_offset : 0));
    if (coef_staged && any) {
        const int* rows = a.coef + (long)o_lo * a.ksize;
        const int n = (o_hi - o_lo) * a.ksize;
        for (int idx = tid; idx < n; idx += RS_THREADS) staged_coef[idx] = rows[idx];
    }
    __syncthreads();

    u8* dst_t = a.dst + (long)t * a.dst_frame;
    const int outputs = ncl * nco;
    for (int idx = tid; idx < outputs; idx += RS_THREADS) {
        const int i = LINES_INNER ? idx % ncl : idx / nco;
        const int j = LINES_INNER ? idx / ncl : idx % nco;
        const int l = cl0 + i - a.off_line, o = co0 + j - a.off_out;
        uint32_t out[C];
        if (l >= 0 && l < a.lines && o >= 0 && o < a.out_size) {
            const int x = min(max(a.bounds[2 * o], 0), a.in_size);
            const int n = min(max(a.bounds[2 * o + 1], 0), min(a.ksize, a.in_size - x));
            const int* k = a.coef + (long)o * a.ksize;
            const int* ks = staged_coef + (o - o_lo) * a.ksize;
            uint32_t acc[C];                                             // unsigned: the wrap of the reference's 32-bit sum, without UB
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 1u << 21;
            const int p0 = x - s_lo;
            const bool all_staged = p0 >= 0 && p0 + n <= n_staged;       // the rule; the loop below it is for what did not fit
            if (all_staged) {
                const u8* s = staged_px + (LINES_INNER ? p0 * nl + (l - l_lo) : (l - l_lo) * n_staged + p0) * C;
                const int step = (LINES_INNER ? nl : 1) * C;
                if (coef_staged) taps<C>(acc, s, step, ks, n);
                else taps<C>(acc, s, step, k, n);
            }
            for (int q = all_staged ? n : 0; q < n; ++q) {
                const uint32_t w = (uint32_t)(coef_staged ? ks[q] : k[q]);
                const int p = p0 + q;
                uint32_t v;
                if (p >= 0 && p < n_staged) {
                    const u8* s = staged_px + (LINES_INNER ? p * nl + (l - l_lo) : (l - l_lo) * n_staged + p) * C;
                    v = s[0];
                    if (C == 3) v |= ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
                } else {
                    const u8* s = src_t + (long)l * a.src_line + (long)(x + q) * a.src_pos;
                    v = fetch<C>(a, s, alpha_t ? alpha_t + (long)l * a.alpha_line + (long)(x + q) * a.alpha_pos : nullptr);
                }
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += ((v >> (8 * c)) & 0xFFu) * w;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] = (uint32_t)min(max((int)acc[c] >> 22, 0), 255);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] = (uint32_t)a.fill;
        }
        u8* d = dst_t + (long)(cl0 + i) * a.dst_line + (long)(co0 + j) * a.dst_pos;
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = (u8)out[c];
    }
}

// ksize of Pillow's precompute_coeffs for a Lanczos (support 3) pass
int frame_ksize(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    const double support = 3.0 * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

}  // namespace

extern "C" int m324_frame_plan(int in_size, int out_size, int lines, int channels, int frames, long* scratch_bytes) {
    M324_REQUIRE(in_size > 0 && out_size > 0 && lines > 0 && frames > 0,
                 "m324_frame_plan: sizes must be positive (in_size=%d out_size=%d lines=%d frames=%d)", in_size, out_size, lines, frames);
    M324_REQUIRE(channels == 1 || channels == 3, "m324_frame_plan: channels must be 1 or 3, got %d", channels);
    M324_REQUIRE(in_size <= M324_FRAME_MAX_SIDE && out_size <= M324_FRAME_MAX_SIDE && lines <= M324_FRAME_MAX_SIDE,
                 "m324_frame_plan: a side of at most %d pixels is supported (in_size=%d out_size=%d lines=%d)", M324_FRAME_MAX_SIDE, in_size,
                 out_size, lines);
    if (scratch_bytes) *scratch_bytes = (long)frames * lines * out_size * channels;
    return frame_ksize(in_size, out_size);
}

extern "C" int m324_frame_mask(const unsigned char* src, long src_frame, long src_pitch, int src_pixel, const unsigned char* alpha,
                               long alpha_frame, long alpha_pitch, int alpha_pixel, int frames, int height, int width, int mode, int threshold,
                               const unsigned char* table, unsigned char* masked, unsigned char* mask, int* boxes, void* stream) {
    M324_REQUIRE(src && boxes, "m324_frame_mask: null src or boxes");
    M324_REQUIRE(frames > 0 && height > 0 && width > 0, "m324_frame_mask: sizes must be positive (frames=%d height=%d width=%d)", frames, height,
                 width);
    M324_REQUIRE(src_pixel == 3 || src_pixel == 4, "m324_frame_mask: the pixel stride is 3 or 4 bytes, got %d", src_pixel);
    M324_REQUIRE(src_pitch >= (long)width * src_pixel - (src_pixel - 3) && src_frame >= 0 && (frames == 1 || src_frame >= (long)height * src_pitch),
                 "m324_frame_mask: source strides too short (frame=%ld pitch=%ld pixel=%d for %d x %d)", src_frame, src_pitch, src_pixel, width,
                 height);
    if (!alpha) {
        M324_REQUIRE(src_pixel == 4, "m324_frame_mask: without an alpha plane the source is RGBA (pixel stride 4), got %d", src_pixel);
        M324_REQUIRE(src_pitch >= (long)width * 4, "m324_frame_mask: source strides too short (pitch=%ld for %d RGBA pixels)", src_pitch, width);
        alpha = src + 3;
        alpha_frame = src_frame; alpha_pitch = src_pitch; alpha_pixel = 4;
    } else {
        M324_REQUIRE(alpha_pixel >= 1 && alpha_pitch >= (long)(width - 1) * alpha_pixel + 1 && alpha_frame >= 0 &&
                         (frames == 1 || alpha_frame >= (long)height * alpha_pitch),
                     "m324_frame_mask: alpha strides too short (frame=%ld pitch=%ld pixel=%d for %d x %d)", alpha_frame, alpha_pitch, alpha_pixel,
                     width, height);
    }
    M324_REQUIRE(mode == M324_FRAME_THRESHOLD || mode == M324_FRAME_SOFT, "m324_frame_mask: mode must be %d (threshold) or %d (soft), got %d",
                 M324_FRAME_THRESHOLD, M324_FRAME_SOFT, mode);
    M324_REQUIRE(mode != M324_FRAME_THRESHOLD || (threshold >= 0 && threshold <= 255), "m324_frame_mask: threshold must be in 0..255, got %d", threshold);
    M324_REQUIRE(mode != M324_FRAME_SOFT || table, "m324_frame_mask: the soft mode needs its 256 x 256 table");
    const int groups = ceil_div(width, MASK_GROUP);
    const long blocks_per_frame = ((long)height * groups + MASK_THREADS - 1) / MASK_THREADS;
    M324_REQUIRE(blocks_per_frame * frames < 2147483647L, "m324_frame_mask: frames * height * width too large");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(frame_box_init_kernel, dim3(ceil_div(frames, MASK_THREADS)), dim3(MASK_THREADS), 0, st, boxes, frames, width, height);
    const dim3 grid((unsigned)(blocks_per_frame * frames)), block(MASK_THREADS);
    if (mode == M324_FRAME_SOFT)
        hipLaunchKernelGGL(frame_mask_kernel<true>, grid, block, 0, st, src, src_frame, src_pitch, src_pixel, alpha, alpha_frame, alpha_pitch,
                           alpha_pixel, height, width, groups, (int)blocks_per_frame, threshold, table, masked, mask, boxes);
    else
        hipLaunchKernelGGL(frame_mask_kernel<false>, grid, block, 0, st, src, src_frame, src_pitch, src_pixel, alpha, alpha_frame, alpha_pitch,
                           alpha_pixel, height, width, groups, (int)blocks_per_frame, threshold, table, masked, mask, boxes);
    M324_CHECK_LAUNCH("m324_frame_mask");
    return M324_OK;
}

extern "C" int m324_frame_resample(const unsigned char* src, long src_frame, long src_pitch, int src_pixel, int src_w, int src_h, int crop_x,
                                   int crop_y, int crop_w, int crop_h, int channels, int frames, int axis, const int* coef, const int* bounds,
                                   int out_size, int ksize, const unsigned char* alpha, long alpha_frame, long alpha_pitch, int alpha_pixel,
                                   int mode, int threshold, const unsigned char* table, unsigned char* dst, long dst_frame, long dst_pitch,
                                   int dst_pixel, int dst_w, int dst_h, int paste_x, int paste_y, int fill, void* stream) {
    M324_REQUIRE(src && coef && bounds && dst, "m324_frame_resample: null src, coef, bounds or dst");
    M324_REQUIRE(channels == 1 || channels == 3, "m324_frame_resample: channels must be 1 or 3, got %d", channels);
    M324_REQUIRE(axis == M324_FRAME_AXIS_X || axis == M324_FRAME_AXIS_Y, "m324_frame_resample: axis must be %d (x) or %d (y), got %d",
                 M324_FRAME_AXIS_X, M324_FRAME_AXIS_Y, axis);
    M324_REQUIRE(frames > 0 && src_w > 0 && src_h > 0 && crop_w > 0 && crop_h > 0 && out_size > 0 && ksize > 0 && dst_w > 0 && dst_h > 0,
                 "m324_frame_resample: sizes must be positive (frames=%d src=%dx%d crop=%dx%d out_size=%d ksize=%d dst=%dx%d)", frames, src_w,
                 src_h, crop_w, crop_h, out_size, ksize, dst_w, dst_h);
    M324_REQUIRE(crop_x >= 0 && crop_y >= 0 && crop_x <= src_w - crop_w && crop_y <= src_h - crop_h,
                 "m324_frame_resample: the crop (%d, %d) + %d x %d leaves the %d x %d source", crop_x, crop_y, crop_w, crop_h, src_w, src_h);
    const int in_size = axis == M324_FRAME_AXIS_X ? crop_w : crop_h;
    const int lines = axis == M324_FRAME_AXIS_X ? crop_h : crop_w;
    M324_REQUIRE(in_size <= M324_FRAME_MAX_SIDE && out_size <= M324_FRAME_MAX_SIDE && lines <= M324_FRAME_MAX_SIDE && dst_w <= M324_FRAME_MAX_SIDE &&
                     dst_h <= M324_FRAME_MAX_SIDE && ksize <= 6 * M324_FRAME_MAX_SIDE + 3,
                 "m324_frame_resample: a side of at most %d pixels is supported (in_size=%d out_size=%d lines=%d dst=%dx%d ksize=%d)",
                 M324_FRAME_MAX_SIDE, in_size, out_size, lines, dst_w, dst_h, ksize);
    M324_REQUIRE(src_pixel >= channels && src_pitch >= (long)(src_w - 1) * src_pixel + channels && src_frame >= 0 &&
                     (frames == 1 || src_frame >= (long)src_h * src_pitch),
                 "m324_frame_resample: source strides too short (frame=%ld pitch=%ld pixel=%d for %d x %d x %d)", src_frame, src_pitch, src_pixel,
                 src_w, src_h, channels);
    M324_REQUIRE(dst_pixel >= channels && dst_pitch >= (long)(dst_w - 1) * dst_pixel + channels && dst_frame >= 0 &&
                     (frames == 1 || dst_frame >= (long)dst_h * dst_pitch),
                 "m324_frame_resample: destination strides too short (frame=%ld pitch=%ld pixel=%d for %d x %d x %d)", dst_frame, dst_pitch,
                 dst_pixel, dst_w, dst_h, channels);
    M324_REQUIRE(mode >= M324_FRAME_NONE && mode <= M324_FRAME_BINARY, "m324_frame_resample: unknown masking mode %d", mode);
    if (mode == M324_FRAME_NONE) {
        alpha = nullptr;
    } else {
        M324_REQUIRE(alpha && alpha_pixel >= 1 && alpha_pitch >= (long)(src_w - 1) * alpha_pixel + 1 && alpha_frame >= 0 &&
                         (frames == 1 || alpha_frame >= (long)src_h * alpha_pitch),
                     "m324_frame_resample: a masking mode needs an alpha plane with strides that hold it (frame=%ld pitch=%ld pixel=%d)", alpha_frame,
                     alpha_pitch, alpha_pixel);
        M324_REQUIRE(mode == M324_FRAME_SOFT || (threshold >= 0 && threshold <= 255), "m324_frame_resample: threshold must be in 0..255, got %d",
                     threshold);
        M324_REQUIRE(mode != M324_FRAME_SOFT || table, "m324_frame_resample: the soft mode needs its 256 x 256 table");
    }
    const int res_w = axis == M324_FRAME_AXIS_X ? out_size : crop_w, res_h = axis == M324_FRAME_AXIS_X ? crop_h : out_size;
    M324_REQUIRE(paste_x >= 0 && paste_y >= 0 && paste_x <= dst_w - res_w && paste_y <= dst_h - res_h,
                 "m324_frame_resample: the result %d x %d pasted at (%d, %d) leaves the %d x %d destination", res_w, res_h, paste_x, paste_y, dst_w,
                 dst_h);
    M324_REQUIRE(fill >= -1 && fill <= 255, "m324_frame_resample: fill must be -1 (region only) or 0..255, got %d", fill);

    PassArgs a;
    a.coef = coef; a.bounds = bounds; a.table = table;
    a.mode = mode; a.threshold = threshold; a.in_size = in_size; a.out_size = out_size; a.ksize = ksize; a.fill = fill < 0 ? 0 : fill;
    a.src = src + (long)crop_y * src_pitch + (long)crop_x * src_pixel;
    a.src_frame = src_frame;
    a.alpha = alpha ? alpha + (long)crop_y * alpha_pitch + (long)crop_x * alpha_pixel : nullptr;
    a.alpha_frame = alpha_frame;
    a.dst = dst; a.dst_frame = dst_frame;
    int C = channels;
    int canvas_lines, canvas_out;
    if (axis == M324_FRAME_AXIS_X) {
        a.lines = lines;
        a.src_line = src_pitch; a.src_pos = src_pixel; a.alpha_line = alpha_pitch; a.alpha_pos = alpha_pixel;
        a.dst_line = dst_pitch; a.dst_pos = dst_pixel;
        a.off_line = paste_y; a.off_out = paste_x;
        canvas_lines = dst_h; canvas_out = dst_w;
    } else if (mode == M324_FRAME_NONE && src_pixel == channels && dst_pixel == channels) {
        // dense pixels and no masking: every BYTE of a row is a line of its own, and neighbouring lanes move neighbouring bytes
        a.lines = lines * channels;
        a.src_line = 1; a.src_pos = src_pitch; a.alpha_line = 0; a.alpha_pos = 0;
        a.dst_line = 1; a.dst_pos = dst_pitch;
        a.off_line = paste_x * channels; a.off_out = paste_y;
        canvas_lines = dst_w * channels; canvas_out = dst_h;
        C = 1;
    } else {
        a.lines = lines;
        a.src_line = src_pixel; a.src_pos = src_pitch; a.alpha_line = alpha_pixel; a.alpha_pos = alpha_pitch;
        a.dst_line = dst_pixel; a.dst_pos = dst_pitch;
        a.off_line = paste_x; a.off_out = paste_y;
        canvas_lines = dst_w; canvas_out = dst_h;
    }
    if (fill >= 0) {
        a.c0_line = 0; a.c1_line = canvas_lines; a.c0_out = 0; a.c1_out = canvas_out;
    } else {
        a.c0_line = a.off_line; a.c1_line = a.off_line + a.lines; a.c0_out = a.off_out; a.c1_out = a.off_out + out_size;
    }
    // Tiles: as many outputs per workgroup as keep the span they read inside the LDS budget.  An output reads at most
    // 2 * support + 1 positions around (o + 0.5) * scale, so `n` neighbouring outputs read at most (n - 1) * scale + 2 * support + 2.
    const double scale = (double)in_size / (double)out_size;
    const double support = 3.0 * (scale < 1.0 ? 1.0 : scale);
    const bool lines_inner = axis == M324_FRAME_AXIS_Y;
    int tile_out = std::min(a.c1_out - a.c0_out, lines_inner ? 64 : 128);
    int tile_lines = lines_inner ? std::min(a.c1_line - a.c0_line, 64) : std::min(a.c1_line - a.c0_line, std::max(1, 512 / tile_out));
    long span = 0;
    for (;;) {
        const double need = (tile_out - 1) * scale + 2.0 * support + 2.0;
        span = need < (double)in_size ? (long)need + 1 : in_size;
        if (span > in_size) span = in_size;
        if (span * tile_lines * C <= RS_LDS_BYTES) break;
        if (!lines_inner && tile_lines > 1) tile_lines = (tile_lines + 1) / 2;
        else if (tile_out > 1) tile_out = (tile_out + 1) / 2;
        else if (tile_lines > 1) tile_lines = (tile_lines + 1) / 2;
        else break;                                                      // one line, one output: in_size * C <= RS_LDS_BYTES
    }
    a.tile_lines = tile_lines; a.tile_out = tile_out;
    a.tiles_lines = ceil_div(a.c1_line - a.c0_line, tile_lines);
    a.tiles_out = ceil_div(a.c1_out - a.c0_out, tile_out);
    long lds_bytes = std::min<long>(RS_LDS_BYTES, (span * tile_lines * C + 15) / 16 * 16);
    a.lds_pixels = (int)(lds_bytes / C);
    a.coef_offset = -1;
    const long coef_bytes = (long)tile_out * ksize * 4;
    if (!lines_inner && lds_bytes + coef_bytes <= RS_LDS_BYTES) {       // the tile's coefficient rows behind the samples
        a.coef_offset = (int)lds_bytes;
        lds_bytes += coef_bytes;
    }
    const long blocks = (long)frames * a.tiles_lines * a.tiles_out;
    M324_REQUIRE(blocks < 2147483647L, "m324_frame_resample: frames * tiles too large");
    const dim3 grid((unsigned)blocks), block(RS_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (C == 3) {
        if (lines_inner) hipLaunchKernelGGL((frame_resample_kernel<3, true>), grid, block, (size_t)lds_bytes, st, a);
        else hipLaunchKernelGGL((frame_resample_kernel<3, false>), grid, block, (size_t)lds_bytes, st, a);
    } else {
        if (lines_inner) hipLaunchKernelGGL((frame_resample_kernel<1, true>), grid, block, (size_t)lds_bytes, st, a);
        else hipLaunchKernelGGL((frame_resample_kernel<1, false>), grid, block, (size_t)lds_bytes, st, a);
    }
    M324_CHECK_LAUNCH("m324_frame_resample");
    return M324_OK;
}
