// Mesh clip renderer (gfx950): an orthographic, z-buffered triangle rasterizer over every frame of a clip with one topology, and
// the shaded frames, face-id and depth buffers behind it -- the last stage after the forward pass (pcd_moved in, pictures out).
// replaces: nothing the reference can run here; it renders through Blender (utils/render.py) and its only rasterizer is CUDA.
//
// The arithmetic IS the contract (include/m324.h spells it out and the test model is written from there): every decision that
// picks the triangle owning a pixel is made in integers -- snapped subpixel vertices, int64 edge functions, an orientation-free
// top-left rule, an integer depth -- and ownership is settled by a 64-bit atomic min over (depth, face index).  Min commutes, so
// the result depends on no arrival order, grid shape, CU count or queue order.  The fp32 part (projection, barycentrics, shading)
// is compiled without contraction and divides / takes roots with the correctly rounded intrinsics.  The second half of the file
// adds a mip-mapped texture and supersampling under the same rules (m324_texture_*, m324_render_shade_tex).
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr long ALIGN = 256;                              // every scratch region starts on a 256-byte boundary
constexpr unsigned long long EMPTY_KEY = ~0ULL;

struct View {
    float m[12];                                         // row-major 3 x 4
};

// Regions of the scratch buffer, in this order: queue counter, keys, projected vertices, view-space positions, queue.
struct Layout {
    long counter, keys, proj, view, queue, total;
};

inline long round_up(long v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

inline Layout layout_of(int n_vertices, int n_faces, int frames, int size) {
    Layout l;
    l.counter = 0;
    l.keys = ALIGN;
    l.proj = l.keys + round_up((long)frames * size * size * 8);
    l.view = l.proj + round_up((long)frames * n_vertices * 16);
    l.queue = l.view + round_up((long)frames * n_vertices * 12);
    l.total = l.queue + round_up((long)frames * n_faces * 4);
    return l;
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }   // false for a NaN as well

// One lane = one (frame, vertex).  proj[g] = (x_sub, y_sub, z_q, valid); view[g] = the fp32 view-space position.
__global__ __launch_bounds__(THREADS) void render_project_kernel(const float* __restrict__ vertices, long stride_t, int n_vertices, long total,
                                                                 View view, float scale, int4* __restrict__ proj, float* __restrict__ pos) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= total) return;
    const long t = g / n_vertices, v = g % n_vertices;
    const float* src = vertices + t * stride_t + v * 3;
    const float x = src[0], y = src[1], z = src[2];
    float p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = ((view.m[r * 4] * x + view.m[r * 4 + 1] * y) + view.m[r * 4 + 2] * z) + view.m[r * 4 + 3];
    int4 q = make_int4(0, 0, 0, 0);
    if (finitef(p[0]) && finitef(p[1]) && finitef(p[2])) {
        q.x = (int)rintf(clampf((p[0] + 0.5f) * scale, -131072.f, 131072.f));
        q.y = (int)rintf(clampf((0.5f - p[1]) * scale, -131072.f, 131072.f));
        q.z = (int)rintf(clampf((1.0f - p[2]) * 4194304.f, 0.f, 8388607.f));
        q.w = 1;
    }
    proj[g] = q;
    pos[g * 3] = p[0];
    pos[g * 3 + 1] = p[1];
    pos[g * 3 + 2] = p[2];
}

// The integer form of one triangle: edge functions w_i = A_i X + B_i Y + C_i, positive inside, w_0 + w_1 + w_2 = area2 > 0.
struct Tri {
    int A[3], B[3];
    long long C[3];
    long long area2;
    int z[3];
    int x0, x1, y0, y1;                                  // pixels whose centres can be inside, clipped to the screen (inclusive)
};

// false: nothing to draw (an index out of range, an invalid vertex, no area, or no pixel centre inside the bounding box)
__device__ __forceinline__ bool setup_tri(const int* __restrict__ faces, long f, int n_vertices, const int4* __restrict__ proj, int size, Tri& t) {
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)n_vertices || (unsigned)i1 >= (unsigned)n_vertices || (unsigned)i2 >= (unsigned)n_vertices) return false;
    const int4 v[3] = {proj[i0], proj[i1], proj[i2]};
    if (!(v[0].w & v[1].w & v[2].w)) return false;
    long long area2 = (long long)(v[1].x - v[0].x) * (v[2].y - v[0].y) - (long long)(v[2].x - v[0].x) * (v[1].y - v[0].y);
    if (area2 == 0) return false;
    const int s = area2 < 0 ? -1 : 1;
    t.area2 = area2 * s;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const int a = v[j].y - v[k].y, b = v[k].x - v[j].x;
        t.A[i] = a * s;
        t.B[i] = b * s;
        t.C[i] = -((long long)a * v[j].x + (long long)b * v[j].y) * s;
        t.z[i] = v[i].z;
    }
    const int xmin = min(v[0].x, min(v[1].x, v[2].x)), xmax = max(v[0].x, max(v[1].x, v[2].x));
    const int ymin = min(v[0].y, min(v[1].y, v[2].y)), ymax = max(v[0].y, max(v[1].y, v[2].y));
    t.x0 = max((xmin + 7) >> 4, 0);                      // first px with 16 px + 8 >= xmin (an arithmetic shift: floor)
    t.x1 = min((xmax - 8) >> 4, size - 1);               // last px with 16 px + 8 <= xmax
    t.y0 = max((ymin + 7) >> 4, 0);
    t.y1 = min((ymax - 8) >> 4, size - 1);
    return t.x0 <= t.x1 && t.y0 <= t.y1;
}

__device__ __forceinline__ bool edge_owns(long long w, int A, int B) { return w > 0 || (w == 0 && (A > 0 || (A == 0 && B > 0))); }

// Pixel (px, py) of one triangle: the coverage test, the depth, the atomic min.  (px, py) is inside the screen.
__device__ __forceinline__ void raster_pixel(const Tri& t, int px, int py, int size, unsigned face, unsigned long long* __restrict__ keys) {
    const long long X = 16 * px + 8, Y = 16 * py + 8;
    const long long w0 = t.A[0] * X + t.B[0] * Y + t.C[0];
    const long long w1 = t.A[1] * X + t.B[1] * Y + t.C[1];
    const long long w2 = t.A[2] * X + t.B[2] * Y + t.C[2];
    if (!(edge_owns(w0, t.A[0], t.B[0]) && edge_owns(w1, t.A[1], t.B[1]) && edge_owns(w2, t.A[2], t.B[2]))) return;
    const long long zp = (w0 * t.z[0] + w1 * t.z[1] + w2 * t.z[2]) / t.area2;
    const unsigned long long key = ((unsigned long long)zp << 32) | face;
    unsigned long long* slot = keys + (long)py * size + px;
    // a key only ever falls, so a stale read can only let a needless atomic through, never hold a needed one back
    if (key < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, key);
}

// One lane = one (frame, face).  A triangle whose box holds at most big_pixels pixels is drawn by its lane; the others go to the
// queue: one counter add per wave for all its lanes that queue (the ballot is taken where the whole wave has reconverged).
__global__ __launch_bounds__(THREADS) void render_small_kernel(const int* __restrict__ faces, int n_faces, int n_vertices, long total, int size,
                                                               int big_pixels, const int4* __restrict__ proj,
                                                               unsigned long long* __restrict__ keys, unsigned* __restrict__ counter,
                                                               unsigned* __restrict__ queue) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    bool queued = false;
    if (g < total) {
        const long frame = g / n_faces, f = g % n_faces;
        Tri t;
        if (setup_tri(faces, f, n_vertices, proj + frame * n_vertices, size, t)) {
            const long box = (long)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1);
            if (box > big_pixels) {
                queued = true;
            } else {
                unsigned long long* k = keys + frame * size * size;
                for (int py = t.y0; py <= t.y1; ++py)
                    for (int px = t.x0; px <= t.x1; ++px) raster_pixel(t, px, py, size, (unsigned)f, k);
            }
        }
    }
    const unsigned long long mask = __ballot(queued);
    if (mask == 0) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(mask));
    base = __shfl(base, leader, 64);
    if (queued) queue[base + __popcll(mask & ((1ULL << lane) - 1ULL))] = (unsigned)g;
}

// One workgroup = one queue entry at a time (a grid-stride walk over the entries the first pass left), lanes striding over the box.
__global__ __launch_bounds__(THREADS) void render_queue_kernel(const int* __restrict__ faces, int n_faces, int n_vertices, long total, int size,
                                                               const int4* __restrict__ proj, unsigned long long* __restrict__ keys,
                                                               const unsigned* __restrict__ counter, const unsigned* __restrict__ queue) {
    const long count = min((long)*counter, total);
    for (long e = blockIdx.x; e < count; e += gridDim.x) {
        const long g = queue[e];
        if (g >= total) continue;
        const long frame = g / n_faces, f = g % n_faces;
        Tri t;
        if (!setup_tri(faces, f, n_vertices, proj + frame * n_vertices, size, t)) continue;
        unsigned long long* k = keys + frame * size * size;
        const int bw = t.x1 - t.x0 + 1;
        const int n = bw * (t.y1 - t.y0 + 1);
        for (int i = threadIdx.x; i < n; i += THREADS) raster_pixel(t, t.x0 + i % bw, t.y0 + i / bw, size, (unsigned)f, k);
    }
}

// One lane = one pixel of one frame: background, or the barycentrics of the owning face, its albedo, its normal, the byte.
template <bool SMOOTH>
__global__ __launch_bounds__(THREADS) void render_shade_kernel(const int* __restrict__ faces, int n_faces, int n_vertices, long total, int size,
                                                               const unsigned long long* __restrict__ keys, const int4* __restrict__ proj,
                                                               const float* __restrict__ pos, const float* __restrict__ colors,
                                                               const float* __restrict__ normals, long normal_stride_t, View view,
                                                               float ambient, int bg0, int bg1, int bg2, unsigned char* __restrict__ rgb,
                                                               int* __restrict__ face_out, int* __restrict__ depth_out) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= total) return;
    const long pixels = (long)size * size;
    const long frame = g / pixels;
    const int at = (int)(g % pixels), py = at / size, px = at % size;
    const unsigned long long key = keys[g];
    int face = -1, depth = -1;
    int out[3] = {bg0, bg1, bg2};
    Tri t;
    if (key != EMPTY_KEY && (key & 0xffffffffULL) < (unsigned long long)n_faces && setup_tri(faces, (long)(key & 0xffffffffULL), n_vertices, proj + frame * n_vertices, size, t)) {
        face = (int)(key & 0xffffffffULL);
        depth = (int)(key >> 32);
        const long i[3] = {faces[(long)face * 3], faces[(long)face * 3 + 1], faces[(long)face * 3 + 2]};
        const long long X = 16 * px + 8, Y = 16 * py + 8;
        const float area = (float)(double)t.area2;       // |values| < 2^53: exact in fp64, so one rounding to fp32
        float b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) b[k] = __fdiv_rn((float)(double)(t.A[k] * X + t.B[k] * Y + t.C[k]), area);
        float n[3];
        if (SMOOTH) {
            const float* vn = normals + frame * normal_stride_t;
            float m[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] = (b[0] * vn[i[0] * 3 + c] + b[1] * vn[i[1] * 3 + c]) + b[2] * vn[i[2] * 3 + c];
#pragma unroll
            for (int r = 0; r < 3; ++r) n[r] = (view.m[r * 4] * m[0] + view.m[r * 4 + 1] * m[1]) + view.m[r * 4 + 2] * m[2];
        } else {
            const float* p = pos + frame * n_vertices * 3;
            float e1[3], e2[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                e1[c] = p[i[1] * 3 + c] - p[i[0] * 3 + c];
                e2[c] = p[i[2] * 3 + c] - p[i[0] * 3 + c];
            }
            n[0] = e1[1] * e2[2] - e1[2] * e2[1];
            n[1] = e1[2] * e2[0] - e1[0] * e2[2];
            n[2] = e1[0] * e2[1] - e1[1] * e2[0];
        }
        const float len = __fsqrt_rn((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        const float l = (len > 0.f && finitef(len)) ? __fdiv_rn(fabsf(n[2]), len) : 0.f;
        const float shade = ambient + (1.0f - ambient) * l;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float albedo = colors ? (b[0] * colors[i[0] * 3 + c] + b[1] * colors[i[1] * 3 + c]) + b[2] * colors[i[2] * 3 + c] : 0.8f;
            float v = albedo * shade;
            v = v > 0.f ? v : 0.f;                       // a NaN counts as 0
            v = v < 1.f ? v : 1.f;
            out[c] = (int)floorf(v * 255.f + 0.5f);
        }
    }
    if (rgb) {
        rgb[g * 3] = (unsigned char)out[0];
        rgb[g * 3 + 1] = (unsigned char)out[1];
        rgb[g * 3 + 2] = (unsigned char)out[2];
    }
    if (face_out) face_out[g] = face;
    if (depth_out) depth_out[g] = depth;
}

// Everything the entry points share: sizes first (no HIP call before they pass), then the scratch buffer against the plan.
int check_sizes(const char* who, int n_vertices, int n_faces, int frames, int size) {
    M324_REQUIRE(size >= 1 && size <= M324_RENDER_MAX_SIDE, "%s: size must be in 1..%d, got %d", who, M324_RENDER_MAX_SIDE, size);
    M324_REQUIRE(frames >= 1 && n_vertices >= 1 && n_faces >= 0, "%s: need frames >= 1, n_vertices >= 1, n_faces >= 0 (frames=%d n_vertices=%d n_faces=%d)",
                 who, frames, n_vertices, n_faces);
    M324_REQUIRE((long)frames * n_faces < 2147483647L && (long)frames * n_vertices < 2147483647L,
                 "%s: frames * n_faces and frames * n_vertices must stay below 2^31 (frames=%d n_vertices=%d n_faces=%d): render fewer frames per call", who,
                 frames, n_vertices, n_faces);
    return M324_OK;
}

int check_scratch(const char* who, const Layout& l, const void* scratch, long scratch_bytes) {
    M324_REQUIRE(scratch && scratch_bytes >= l.total, "%s: needs %ld scratch bytes (m324_render_plan), got %ld", who, l.total, scratch ? scratch_bytes : 0L);
    M324_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-byte aligned", who);
    return M324_OK;
}

}  // namespace

extern "C" int m324_render_plan(int n_vertices, int n_faces, int frames, int size, long* scratch_bytes) {
    const int rc = check_sizes("m324_render_plan", n_vertices, n_faces, frames, size);
    if (rc != M324_OK) return rc;
    if (scratch_bytes) *scratch_bytes = layout_of(n_vertices, n_faces, frames, size).total;
    return M324_OK;
}

extern "C" int m324_render_project(const float* vertices, long stride_t, int n_vertices, int n_faces, int frames, const float* view, int size,
                                   void* scratch, long scratch_bytes, void* stream) {
    M324_REQUIRE(vertices && view && scratch, "m324_render_project: null vertices, view or scratch");
    int rc = check_sizes("m324_render_project", n_vertices, n_faces, frames, size);
    if (rc != M324_OK) return rc;
    M324_REQUIRE(stride_t >= 0, "m324_render_project: stride_t must not be negative, got %ld", stride_t);
    const Layout l = layout_of(n_vertices, n_faces, frames, size);
    rc = check_scratch("m324_render_project", l, scratch, scratch_bytes);
    if (rc != M324_OK) return rc;
    View m;
    for (int i = 0; i < 12; ++i) m.m[i] = view[i];
    char* base = (char*)scratch;
    const long total = (long)frames * n_vertices;
    hipLaunchKernelGGL(render_project_kernel, dim3(ceil_div(total, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, vertices, stride_t, n_vertices,
                       total, m, (float)(16 * size), (int4*)(base + l.proj), (float*)(base + l.view));
    M324_CHECK_LAUNCH("m324_render_project");
    return M324_OK;
}

extern "C" int m324_render_raster(const int* faces, int n_faces, int n_vertices, int frames, int size, int big_pixels, void* scratch,
                                  long scratch_bytes, void* stream) {
    M324_REQUIRE(scratch && (faces || n_faces == 0), "m324_render_raster: null faces or scratch");
    int rc = check_sizes("m324_render_raster", n_vertices, n_faces, frames, size);
    if (rc != M324_OK) return rc;
    M324_REQUIRE(big_pixels >= 0, "m324_render_raster: big_pixels must not be negative, got %d", big_pixels);
    const Layout l = layout_of(n_vertices, n_faces, frames, size);
    rc = check_scratch("m324_render_raster", l, scratch, scratch_bytes);
    if (rc != M324_OK) return rc;
    char* base = (char*)scratch;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)(base + l.keys);
    unsigned* counter = (unsigned*)(base + l.counter);
    unsigned* queue = (unsigned*)(base + l.queue);
    const int4* proj = (const int4*)(base + l.proj);
    hipError_t e = hipMemsetAsync(keys, 0xFF, (size_t)frames * size * size * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(counter, 0, ALIGN, st);
    if (e != hipSuccess) M324_FAIL(M324_ERR_HIP, "m324_render_raster: %s", hipGetErrorString(e));
    const long total = (long)frames * n_faces;
    if (total > 0) {
        hipLaunchKernelGGL(render_small_kernel, dim3(ceil_div(total, THREADS)), dim3(THREADS), 0, st, faces, n_faces, n_vertices, total, size,
                           big_pixels, proj, keys, counter, queue);
        // as many workgroups as the chip holds a few times over, never more than there can be entries
        const long chip = 16L * m324::cu_count();
        const long groups = total < chip ? total : chip;
        hipLaunchKernelGGL(render_queue_kernel, dim3((unsigned)groups), dim3(THREADS), 0, st, faces, n_faces, n_vertices, total, size, proj, keys,
                           counter, queue);
    }
    M324_CHECK_LAUNCH("m324_render_raster");
    return M324_OK;
}

extern "C" int m324_render_shade(const int* faces, int n_faces, int n_vertices, int frames, int size, const float* colors, const float* normals,
                                 long normal_stride_t, const float* view, float ambient, int background, unsigned char* rgb, int* face,
                                 int* depth, void* scratch, long scratch_bytes, void* stream) {
    M324_REQUIRE(scratch && view && (faces || n_faces == 0), "m324_render_shade: null faces, view or scratch");
    M324_REQUIRE(rgb || face || depth, "m324_render_shade: null rgb, face and depth: nothing to write");
    int rc = check_sizes("m324_render_shade", n_vertices, n_faces, frames, size);
    if (rc != M324_OK) return rc;
    M324_REQUIRE(normal_stride_t >= 0 && ambient >= 0.f && ambient <= 1.f && background >= 0 && background <= 0xffffff,
                 "m324_render_shade: need normal_stride_t >= 0, ambient in [0, 1], background = 0xBBGGRR (normal_stride_t=%ld ambient=%g background=%d)",
                 normal_stride_t, (double)ambient, background);
    const Layout l = layout_of(n_vertices, n_faces, frames, size);
    rc = check_scratch("m324_render_shade", l, scratch, scratch_bytes);
    if (rc != M324_OK) return rc;
    View m;
    for (int i = 0; i < 12; ++i) m.m[i] = view[i];
    char* base = (char*)scratch;
    const long total = (long)frames * size * size;
    const dim3 grid(ceil_div(total, THREADS)), block(THREADS);
    const unsigned long long* keys = (const unsigned long long*)(base + l.keys);
    const int4* proj = (const int4*)(base + l.proj);
    const float* pos = (const float*)(base + l.view);
    const int bg0 = background & 255, bg1 = (background >> 8) & 255, bg2 = (background >> 16) & 255;
    if (normals)
        hipLaunchKernelGGL(render_shade_kernel<true>, grid, block, 0, (hipStream_t)stream, faces, n_faces, n_vertices, total, size, keys, proj, pos, colors,
                           normals, normal_stride_t, m, ambient, bg0, bg1, bg2, rgb, face, depth);
    else
        hipLaunchKernelGGL(render_shade_kernel<false>, grid, block, 0, (hipStream_t)stream, faces, n_faces, n_vertices, total, size, keys, proj, pos, colors,
                           normals, normal_stride_t, m, ambient, bg0, bg1, bg2, rgb, face, depth);
    M324_CHECK_LAUNCH("m324_render_shade");
    return M324_OK;
}

// ------------------------------------------------------------------------------------------------ textures and supersampling
// A mip-mapped base-colour texture addressed through per-corner UVs, and ss x ss samples per output pixel resolved by the lane
// that shades them (include/m324.h, "Textured and anti-aliased mesh clips").  The camera is orthographic and UVs interpolate
// affinely, so one level per (frame, face) is the exact isotropic level; it is picked by comparisons against powers of two.
namespace {

// The chain of a texture, passed to the kernels by value: off[l] is level l's offset in 32-bit texels, off[levels] the end.
struct Chain {
    long off[M324_TEXTURE_MAX_LEVELS + 1];
    int levels, w0, h0;
};

inline Chain chain_of(int tex_h, int tex_w) {
    Chain c;
    c.w0 = tex_w;
    c.h0 = tex_h;
    long at = 0;
    int w = tex_w, h = tex_h, l = 0;
    for (;; ++l) {
        c.off[l] = at / 4;
        at += round_up(4L * w * h);
        if (w == 1 && h == 1) break;
        w = w > 1 ? w >> 1 : 1;
        h = h > 1 ? h >> 1 : 1;
    }
    c.levels = l + 1;
    for (int k = c.levels; k <= M324_TEXTURE_MAX_LEVELS; ++k) c.off[k] = at / 4;
    return c;
}

int check_texture(const char* who, int tex_h, int tex_w) {
    M324_REQUIRE(tex_h >= 1 && tex_h <= M324_TEXTURE_MAX_SIDE && tex_w >= 1 && tex_w <= M324_TEXTURE_MAX_SIDE,
                 "%s: texture sides must be in 1..%d, got %d x %d", who, M324_TEXTURE_MAX_SIDE, tex_h, tex_w);
    return M324_OK;
}

// One lane = one texel of level 0: R, G, B and a zero byte.
__global__ __launch_bounds__(THREADS) void texture_pack_kernel(const unsigned char* __restrict__ texels, long total, int channels,
                                                               unsigned* __restrict__ out) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= total) return;
    const unsigned char* p = texels + g * channels;
    out[g] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

// One lane = one texel of level l + 1: the rounded mean of a 2 x 2 block of level l, per byte.
__global__ __launch_bounds__(THREADS) void texture_down_kernel(const unsigned* __restrict__ src, int sw, int sh, unsigned* __restrict__ dst,
                                                               int dw, long total) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= total) return;
    const int x = (int)(g % dw), y = (int)(g / dw);
    const int x0 = min(2 * x, sw - 1), x1 = min(2 * x + 1, sw - 1), y0 = min(2 * y, sh - 1), y1 = min(2 * y + 1, sh - 1);
    const unsigned a = src[(long)y0 * sw + x0], b = src[(long)y0 * sw + x1], c = src[(long)y1 * sw + x0], d = src[(long)y1 * sw + x1];
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 24; k += 8) out |= ((((a >> k) & 255u) + ((b >> k) & 255u) + ((c >> k) & 255u) + ((d >> k) & 255u) + 2u) >> 2) << k;
    dst[g] = out;
}

// What a lane keeps of the face that owns its current sample; rebuilt only when the next sample belongs to another face.
struct FaceState {
    Tri t;
    long i[3];
    float area;
    float shade;                                         // flat shading: constant over the face
    float u[3], v[3];                                    // corner UVs, non-finite components replaced by 0
    int lw, lh;                                          // the level's sides
    long loff;                                           // and its offset in texels
};

template <bool SMOOTH, bool TEX>
__device__ __forceinline__ void face_setup(FaceState& s, int face, const int* __restrict__ faces, int n_vertices, const float* __restrict__ pos_t,
                                           float ambient, const float* __restrict__ face_uvs, const Chain& chain, int last) {
    s.i[0] = faces[(long)face * 3];
    s.i[1] = faces[(long)face * 3 + 1];
    s.i[2] = faces[(long)face * 3 + 2];
    s.area = (float)(double)s.t.area2;                   // |values| < 2^53: exact in fp64, so one rounding to fp32
    if (!SMOOTH) {
        float e1[3], e2[3], n[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            e1[c] = pos_t[s.i[1] * 3 + c] - pos_t[s.i[0] * 3 + c];
            e2[c] = pos_t[s.i[2] * 3 + c] - pos_t[s.i[0] * 3 + c];
        }
        n[0] = e1[1] * e2[2] - e1[2] * e2[1];
        n[1] = e1[2] * e2[0] - e1[0] * e2[2];
        n[2] = e1[0] * e2[1] - e1[1] * e2[0];
        const float len = __fsqrt_rn((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        const float l = (len > 0.f && finitef(len)) ? __fdiv_rn(fabsf(n[2]), len) : 0.f;
        s.shade = ambient + (1.0f - ambient) * l;
    }
    if (TEX) {
        const float* uv = face_uvs + (long)face * 6;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a = uv[2 * k], b = uv[2 * k + 1];
            s.u[k] = finitef(a) ? a : 0.f;
            s.v[k] = finitef(b) ? b : 0.f;
        }
        const float ua2 = fabsf((s.u[1] - s.u[0]) * (s.v[2] - s.v[0]) - (s.u[2] - s.u[0]) * (s.v[1] - s.v[0]));
        const float rho = __fdiv_rn((ua2 * (float)chain.w0) * (float)chain.h0, s.area / 256.0f);
        // while (l < last && rho > 2 * 4^l) ++l, unrolled: the condition is monotone in l, so the highest level whose test
        // passes is where the loop stops.  Constant indices keep the offsets in the kernel's arguments (no table in memory).
        int l = 0;
        long off = chain.off[0];
        float threshold = 2.0f;
#pragma unroll
        for (int k = 1; k < M324_TEXTURE_MAX_LEVELS; ++k) {
            if (k <= last && rho > threshold) {
                l = k;
                off = chain.off[k];
            }
            threshold *= 4.0f;                           // a power of two: exact
        }
        s.lw = max(chain.w0 >> l, 1);
        s.lh = max(chain.h0 >> l, 1);
        s.loff = off;
    }
}

// One lane = one OUTPUT pixel of one frame: it walks its ss x ss samples, shades each as render_shade_kernel does (the albedo
// from the texture when TEX), writes the samples' face and depth, and stores the rounded mean of their bytes.
template <bool SMOOTH, bool TEX>
__global__ __launch_bounds__(THREADS) void render_shade_tex_kernel(const int* __restrict__ faces, int n_faces, int n_vertices, long total, int size,
                                                                   int ss, const unsigned long long* __restrict__ keys,
                                                                   const int4* __restrict__ proj, const float* __restrict__ pos,
                                                                   const float* __restrict__ colors, const float* __restrict__ normals,
                                                                   long normal_stride_t, View view, float ambient, int bg0, int bg1, int bg2,
                                                                   const float* __restrict__ face_uvs, const unsigned* __restrict__ mips,
                                                                   Chain chain, int last, unsigned char* __restrict__ rgb,
                                                                   int* __restrict__ face_out, int* __restrict__ depth_out) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= total) return;
    const int so = size / ss;
    const long out_pixels = (long)so * so;
    const long frame = g / out_pixels;
    const int at = (int)(g % out_pixels), oy = at / so, ox = at % so;
    const int4* proj_t = proj + frame * n_vertices;
    const float* pos_t = pos + frame * n_vertices * 3;
    const long sample0 = frame * size * size;
    FaceState s;
    int current = -1;                                    // the face s describes
    int sum[3] = {0, 0, 0};
    for (int sy = 0; sy < ss; ++sy) {
        for (int sx = 0; sx < ss; ++sx) {
            const int px = ox * ss + sx, py = oy * ss + sy;
            const long at_s = sample0 + (long)py * size + px;
            const unsigned long long key = keys[at_s];
            int face = -1, depth = -1;
            int out[3] = {bg0, bg1, bg2};
            bool owned = key != EMPTY_KEY && (key & 0xffffffffULL) < (unsigned long long)n_faces;
            if (owned) {
                const int f = (int)(key & 0xffffffffULL);
                if (f != current) {
                    owned = setup_tri(faces, (long)f, n_vertices, proj_t, size, s.t);
                    current = -1;
                    if (owned) {
                        face_setup<SMOOTH, TEX>(s, f, faces, n_vertices, pos_t, ambient, face_uvs, chain, last);
                        current = f;
                    }
                }
            }
            if (owned) {
                face = current;
                depth = (int)(key >> 32);
                const long long X = 16 * px + 8, Y = 16 * py + 8;
                float b[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) b[k] = __fdiv_rn((float)(double)(s.t.A[k] * X + s.t.B[k] * Y + s.t.C[k]), s.area);
                float shade = SMOOTH ? 0.f : s.shade;
                if (SMOOTH) {
                    const float* vn = normals + frame * normal_stride_t;
                    float m[3], n[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) m[c] = (b[0] * vn[s.i[0] * 3 + c] + b[1] * vn[s.i[1] * 3 + c]) + b[2] * vn[s.i[2] * 3 + c];
#pragma unroll
                    for (int r = 0; r < 3; ++r) n[r] = (view.m[r * 4] * m[0] + view.m[r * 4 + 1] * m[1]) + view.m[r * 4 + 2] * m[2];
                    const float len = __fsqrt_rn((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
                    const float l = (len > 0.f && finitef(len)) ? __fdiv_rn(fabsf(n[2]), len) : 0.f;
                    shade = ambient + (1.0f - ambient) * l;
                }
                unsigned t00 = 0, t01 = 0, t10 = 0, t11 = 0;
                float fx = 0.f, fy = 0.f;
                if (TEX) {
                    float u = (b[0] * s.u[0] + b[1] * s.u[1]) + b[2] * s.u[2];
                    float v = (b[0] * s.v[0] + b[1] * s.v[1]) + b[2] * s.v[2];
                    u = finitef(u) ? u : 0.f;
                    v = finitef(v) ? v : 0.f;
                    const float uw = u - floorf(u), vw = v - floorf(v);          // in [0, 1]
                    const float x = uw * (float)s.lw - 0.5f, y = (1.0f - vw) * (float)s.lh - 0.5f;
                    const float xf = floorf(x), yf = floorf(y);                  // in [-1, side - 1]
                    fx = x - xf;
                    fy = y - yf;
                    const int x0 = (int)xf, y0 = (int)yf;
                    int c0 = x0 < 0 ? x0 + s.lw : x0, c1 = x0 + 1 >= s.lw ? x0 + 1 - s.lw : x0 + 1;
                    int r0 = y0 < 0 ? y0 + s.lh : y0, r1 = y0 + 1 >= s.lh ? y0 + 1 - s.lh : y0 + 1;
                    // the ranges above already hold; the clamps keep every tap inside the level whatever the arithmetic did
                    c0 = min(max(c0, 0), s.lw - 1);
                    c1 = min(max(c1, 0), s.lw - 1);
                    r0 = min(max(r0, 0), s.lh - 1);
                    r1 = min(max(r1, 0), s.lh - 1);
                    const unsigned* level = mips + s.loff;
                    t00 = level[(long)r0 * s.lw + c0];
                    t01 = level[(long)r0 * s.lw + c1];
                    t10 = level[(long)r1 * s.lw + c0];
                    t11 = level[(long)r1 * s.lw + c1];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float albedo;
                    if (TEX) {
                        const float a00 = (float)((t00 >> (8 * c)) & 255u), a01 = (float)((t01 >> (8 * c)) & 255u);
                        const float a10 = (float)((t10 >> (8 * c)) & 255u), a11 = (float)((t11 >> (8 * c)) & 255u);
                        const float top = a00 + fx * (a01 - a00);
                        const float bot = a10 + fx * (a11 - a10);
                        albedo = __fdiv_rn(top + fy * (bot - top), 255.0f);
                    } else {
                        albedo = colors ? (b[0] * colors[s.i[0] * 3 + c] + b[1] * colors[s.i[1] * 3 + c]) + b[2] * colors[s.i[2] * 3 + c] : 0.8f;
                    }
                    float v = albedo * shade;
                    v = v > 0.f ? v : 0.f;               // a NaN counts as 0
                    v = v < 1.f ? v : 1.f;
                    out[c] = (int)floorf(v * 255.f + 0.5f);
                }
            }
            sum[0] += out[0];
            sum[1] += out[1];
            sum[2] += out[2];
            if (face_out) face_out[at_s] = face;
            if (depth_out) depth_out[at_s] = depth;
        }
    }
    if (rgb) {
        const int half = (ss * ss) >> 1, shift = ss == 1 ? 0 : (ss == 2 ? 2 : 4);
        rgb[g * 3] = (unsigned char)((sum[0] + half) >> shift);
        rgb[g * 3 + 1] = (unsigned char)((sum[1] + half) >> shift);
        rgb[g * 3 + 2] = (unsigned char)((sum[2] + half) >> shift);
    }
}

}  // namespace

extern "C" int m324_texture_plan(int tex_h, int tex_w, int* levels, long* bytes) {
    const int rc = check_texture("m324_texture_plan", tex_h, tex_w);
    if (rc != M324_OK) return rc;
    const Chain c = chain_of(tex_h, tex_w);
    if (levels) *levels = c.levels;
    if (bytes) *bytes = c.off[c.levels] * 4;
    return M324_OK;
}

extern "C" int m324_texture_mips(const unsigned char* texels, int tex_h, int tex_w, int channels, void* mips, long mips_bytes, void* stream) {
    M324_REQUIRE(texels && mips, "m324_texture_mips: null texels or mips");
    const int rc = check_texture("m324_texture_mips", tex_h, tex_w);
    if (rc != M324_OK) return rc;
    M324_REQUIRE(channels == 3 || channels == 4, "m324_texture_mips: channels must be 3 or 4, got %d", channels);
    const Chain c = chain_of(tex_h, tex_w);
    M324_REQUIRE(mips_bytes >= c.off[c.levels] * 4, "m324_texture_mips: needs %ld mips bytes (m324_texture_plan), got %ld", c.off[c.levels] * 4, mips_bytes);
    M324_REQUIRE(((uintptr_t)mips & 3) == 0, "m324_texture_mips: mips must be 4-byte aligned");
    unsigned* base = (unsigned*)mips;
    hipStream_t st = (hipStream_t)stream;
    long total = (long)tex_h * tex_w;
    hipLaunchKernelGGL(texture_pack_kernel, dim3(ceil_div(total, THREADS)), dim3(THREADS), 0, st, texels, total, channels, base);
    int w = tex_w, h = tex_h;
    for (int l = 0; l + 1 < c.levels; ++l) {
        const int dw = w > 1 ? w >> 1 : 1, dh = h > 1 ? h >> 1 : 1;
        total = (long)dw * dh;
        hipLaunchKernelGGL(texture_down_kernel, dim3(ceil_div(total, THREADS)), dim3(THREADS), 0, st, base + c.off[l], w, h, base + c.off[l + 1], dw, total);
        w = dw;
        h = dh;
    }
    M324_CHECK_LAUNCH("m324_texture_mips");
    return M324_OK;
}

extern "C" int m324_render_shade_tex(const int* faces, int n_faces, int n_vertices, int frames, int size, const float* colors, const float* normals,
                                     long normal_stride_t, const float* view, float ambient, int background, const float* face_uvs,
                                     const void* mips, int tex_h, int tex_w, int use_mips, int supersample, unsigned char* rgb, int* face,
                                     int* depth, void* scratch, long scratch_bytes, void* stream) {
    M324_REQUIRE(scratch && view && (faces || n_faces == 0), "m324_render_shade_tex: null faces, view or scratch");
    M324_REQUIRE(rgb || face || depth, "m324_render_shade_tex: null rgb, face and depth: nothing to write");
    int rc = check_sizes("m324_render_shade_tex", n_vertices, n_faces, frames, size);
    if (rc != M324_OK) return rc;
    M324_REQUIRE(normal_stride_t >= 0 && ambient >= 0.f && ambient <= 1.f && background >= 0 && background <= 0xffffff,
                 "m324_render_shade_tex: need normal_stride_t >= 0, ambient in [0, 1], background = 0xBBGGRR (normal_stride_t=%ld ambient=%g background=%d)",
                 normal_stride_t, (double)ambient, background);
    M324_REQUIRE(supersample == 1 || supersample == 2 || supersample == 4, "m324_render_shade_tex: supersample must be 1, 2 or 4, got %d", supersample);
    M324_REQUIRE(size % supersample == 0, "m324_render_shade_tex: size (the sample resolution, %d) must be a multiple of supersample (%d)", size, supersample);
    M324_REQUIRE((face_uvs != nullptr) == (mips != nullptr), "m324_render_shade_tex: face_uvs and mips go together (a texture needs UVs, UVs need a texture)");
    Chain chain = {};
    if (face_uvs) {
        M324_REQUIRE(!colors, "m324_render_shade_tex: a texture and colors are two albedos: give one");
        rc = check_texture("m324_render_shade_tex", tex_h, tex_w);
        if (rc != M324_OK) return rc;
        M324_REQUIRE(((uintptr_t)mips & 3) == 0, "m324_render_shade_tex: mips must be 4-byte aligned");
        chain = chain_of(tex_h, tex_w);
    } else {
        M324_REQUIRE(tex_h == 0 && tex_w == 0, "m324_render_shade_tex: a texture size (%d x %d) without face_uvs and mips", tex_h, tex_w);
    }
    const Layout l = layout_of(n_vertices, n_faces, frames, size);
    rc = check_scratch("m324_render_shade_tex", l, scratch, scratch_bytes);
    if (rc != M324_OK) return rc;
    View m;
    for (int i = 0; i < 12; ++i) m.m[i] = view[i];
    char* base = (char*)scratch;
    const int so = size / supersample;
    const long total = (long)frames * so * so;
    const dim3 grid(ceil_div(total, THREADS)), block(THREADS);
    const unsigned long long* keys = (const unsigned long long*)(base + l.keys);
    const int4* proj = (const int4*)(base + l.proj);
    const float* pos = (const float*)(base + l.view);
    const int bg0 = background & 255, bg1 = (background >> 8) & 255, bg2 = (background >> 16) & 255;
    const int last = (face_uvs && use_mips) ? chain.levels - 1 : 0;
    const unsigned* tex = (const unsigned*)mips;
    hipStream_t st = (hipStream_t)stream;
#define M324_SHADE_TEX(SMOOTH, TEX)                                                                                                              \
    hipLaunchKernelGGL((render_shade_tex_kernel<SMOOTH, TEX>), grid, block, 0, st, faces, n_faces, n_vertices, total, size, supersample, keys, proj, \
                       pos, colors, normals, normal_stride_t, m, ambient, bg0, bg1, bg2, face_uvs, tex, chain, last, rgb, face, depth)
    if (normals && face_uvs) M324_SHADE_TEX(true, true);
    else if (normals) M324_SHADE_TEX(true, false);
    else if (face_uvs) M324_SHADE_TEX(false, true);
    else M324_SHADE_TEX(false, false);
#undef M324_SHADE_TEX
    M324_CHECK_LAUNCH("m324_render_shade_tex");
    return M324_OK;
}
