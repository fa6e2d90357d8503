// Surface sampling kernels (gfx950): the area-weighted CDF of a batch of meshes and the seeded, counter-based draw of surface
// points with face index, face normal and colour -- the device twin of motion324_amd/preprocess.py sample_surface /
// sample_pointcloud_with_albedo (utils/mesh_processing.py:130-191 in the reference: trimesh's sampler plus a Python loop per
// sample for the texture lookup).
//
// The arithmetic IS the contract: for the same (mesh, num, seed) the device draws the samples the host sampler draws.  Every
// fp64 expression below is written in the order numpy evaluates it and the whole file is compiled without contraction (hipcc
// fuses a * b + c by default; numpy never does); square roots and divisions are the correctly rounded ones.  The only place the
// two samplers may part is the order of the CDF's additions: np.cumsum is one sequential chain, the scan here is a fixed nested
// order (include/m324.h) that depends on n_faces alone -- identical on meshes whose partial sums are exact, within a few ulp of
// the total otherwise.  No atomics; nothing depends on the grid, the batch or the CU count.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int SCAN_CHUNK = M324_SURFACE_CHUNK;           // faces per sequential inclusive prefix
constexpr int SCAN_BLOCK = M324_SURFACE_BLOCK;           // faces per workgroup
constexpr int SCAN_CHUNKS = SCAN_BLOCK / SCAN_CHUNK;     // 64: one wave takes the chunk prefixes
constexpr int SCAN_THREADS = 256;
constexpr int SAMPLE_THREADS = 256;                      // samples per work item of m324_surface_sample
static_assert(SCAN_BLOCK % SCAN_CHUNK == 0 && SCAN_CHUNKS <= SCAN_THREADS && SCAN_BLOCK % SCAN_THREADS == 0, "scan geometry");

struct Tri {
    double v0[3], e1[3], e2[3];
};

// e1 = v1 - v0, e2 = v2 - v0.  The vertex indices are the caller's: the Python wrappers check their range before any launch.
__device__ __forceinline__ Tri load_tri(const double* __restrict__ v, const int* __restrict__ faces, int f) {
    const int i0 = faces[(long)f * 3], i1 = faces[(long)f * 3 + 1], i2 = faces[(long)f * 3 + 2];
    Tri t;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        t.v0[c] = v[(long)i0 * 3 + c];
        t.e1[c] = v[(long)i1 * 3 + c] - t.v0[c];
        t.e2[c] = v[(long)i2 * 3 + c] - t.v0[c];
    }
    return t;
}

// np.cross(e1, e2) and np.linalg.norm of it: sqrt((cx*cx + cy*cy) + cz*cz)
__device__ __forceinline__ double cross_norm(const Tri& t, double (&c)[3]) {
    c[0] = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1];
    c[1] = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2];
    c[2] = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
    return __dsqrt_rn((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
}

// One workgroup = one block of SCAN_BLOCK faces of one batch item.  Writes L = W + p (the CDF local to the block) and the
// block's total; surface_offset_kernel adds the exclusive prefix of the totals.
__global__ __launch_bounds__(SCAN_THREADS) void surface_block_kernel(const double* __restrict__ vertices, long stride_v,
                                                                     const int* __restrict__ faces, int n_faces, int n_blocks,
                                                                     double* __restrict__ cdf, double* __restrict__ block_total) {
    __shared__ double p[SCAN_BLOCK];
    __shared__ double w[SCAN_CHUNKS];
    const int blk = blockIdx.x % n_blocks;
    const int b = blockIdx.x / n_blocks;
    const double* v = vertices + (long)b * stride_v;
    const int f0 = blk * SCAN_BLOCK;
    const int cnt = min(SCAN_BLOCK, n_faces - f0);           // >= 1
    const int tid = threadIdx.x;

    for (int e = tid; e < cnt; e += SCAN_THREADS) {
        double c[3];
        p[e] = 0.5 * cross_norm(load_tri(v, faces, f0 + e), c);
    }
    __syncthreads();
    if (tid < SCAN_CHUNKS) {                                 // sequential inclusive prefix inside each chunk of 16
        const int lo = tid * SCAN_CHUNK;
        const int hi = min(cnt, lo + SCAN_CHUNK);
        double run = 0.0;
        for (int e = lo; e < hi; ++e) {
            run = e == lo ? p[e] : run + p[e];
            p[e] = run;
        }
        w[tid] = run;                                        // the chunk's total (unused for a chunk past the end)
    }
    __syncthreads();
    double before = 0.0;                                     // W: sequential exclusive prefix of the chunk totals
    if (tid < SCAN_CHUNKS) {
        for (int k = 0; k < tid; ++k) before = k == 0 ? w[0] : before + w[k];
    }
    __syncthreads();
    if (tid < SCAN_CHUNKS) w[tid] = before;
    __syncthreads();
    double* out = cdf + (long)b * n_faces + f0;
    for (int e = tid; e < cnt; e += SCAN_THREADS) {
        const double L = w[e / SCAN_CHUNK] + p[e];
        out[e] = L;
        if (e == cnt - 1 && block_total) block_total[(long)b * n_blocks + blk] = L;
    }
}

// cdf = B + L, B = sequential exclusive prefix of the block totals.  Block 0 keeps its values (B = 0) and is not launched.
__global__ __launch_bounds__(SCAN_THREADS) void surface_offset_kernel(const double* __restrict__ block_total, int n_faces, int n_blocks,
                                                                      double* __restrict__ cdf) {
    const int blk = 1 + blockIdx.x % (n_blocks - 1);
    const int b = blockIdx.x / (n_blocks - 1);
    const double* tot = block_total + (long)b * n_blocks;
    double B = tot[0];
    for (int k = 1; k < blk; ++k) B = B + tot[k];
    const int f0 = blk * SCAN_BLOCK;
    const int cnt = min(SCAN_BLOCK, n_faces - f0);
    double* out = cdf + (long)b * n_faces + f0;
    for (int e = threadIdx.x; e < cnt; e += SCAN_THREADS) out[e] = B + out[e];
}

// motion324_amd.synth: element j of the stream with seed s, a U[0, 1] value rounded to fp32 (1.0 is possible)
__device__ __forceinline__ double stream_uniform(unsigned long long s, unsigned long long j) {
    unsigned long long z = j * 0xD1342543DE82EF95ULL + s + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z = z ^ (z >> 31);
    return (double)(float)((double)(z >> 11) * (1.0 / 9007199254740992.0));
}

// numpy's float remainder by 1.0: the result carries the sign of the divisor
__device__ __forceinline__ double mod_one(double x) {
    double r = fmod(x, 1.0);
    if (r != 0.0) {
        if (r < 0.0) r = r + 1.0;
    } else {
        r = 0.0;
    }
    return r;
}

// (int)clip(x, 0, n - 1); a NaN lands on 0, so the index is always inside the image
__device__ __forceinline__ int clip_index(double x, int n) {
    if (!(x > 0.0)) return 0;
    const double top = (double)(n - 1);
    return (int)(x < top ? x : top);
}

enum { COLOR_NONE = 0, COLOR_GREY, COLOR_VERTEX, COLOR_TEXTURE };

// One work item = (batch item, tile of SAMPLE_THREADS samples) of a flat grid, one sample per lane: one hash for the face, a
// binary search of the item's CDF row (at most 32 dependent fp64 reads, the first ones shared by every lane and served by the
// L2), two hashes for the barycentric pair, three vertex gathers.
template <int COLOR>
__global__ __launch_bounds__(SAMPLE_THREADS) void surface_sample_kernel(
    const double* __restrict__ vertices, long stride_v, const int* __restrict__ faces, int n_faces, const double* __restrict__ cdf,
    const unsigned long long* __restrict__ seeds, int num, int tiles, float* __restrict__ points, double* __restrict__ points64,
    int* __restrict__ face_index, float* __restrict__ normals, float* __restrict__ colors,
    const unsigned char* __restrict__ vertex_colors, int color_channels, const double* __restrict__ uv,
    const unsigned char* __restrict__ texels, int tex_h, int tex_w) {
    const int b = blockIdx.x / tiles;
    const int i = (blockIdx.x % tiles) * SAMPLE_THREADS + threadIdx.x;
    if (i >= num) return;
    const double* v = vertices + (long)b * stride_v;
    const double* row = cdf + (long)b * n_faces;
    const unsigned long long seed_face = seeds[(long)b * 2], seed_bary = seeds[(long)b * 2 + 1];

    const double target = stream_uniform(seed_face, (unsigned long long)i) * row[n_faces - 1];
    int lo = 0, hi = n_faces;                                // first index with cdf > target: searchsorted(side="right")
    for (int step = 0; step < 32 && lo < hi; ++step) {       // n_faces < 2^31: 31 halvings empty the range
        const int mid = lo + ((hi - lo) >> 1);
        if (row[mid] > target) hi = mid; else lo = mid + 1;  // a NaN compares false: the range still shrinks
    }
    const int f = min(max(lo, 0), n_faces - 1);

    double r0 = stream_uniform(seed_bary, 2ULL * (unsigned long long)i);
    double r1 = stream_uniform(seed_bary, 2ULL * (unsigned long long)i + 1ULL);
    if (r0 + r1 > 1.0) {
        r0 = 1.0 - r0;
        r1 = 1.0 - r1;
    }
    const Tri t = load_tri(v, faces, f);
    const long o = ((long)b * num + i) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double x = (t.v0[c] + r0 * t.e1[c]) + r1 * t.e2[c];
        points[o + c] = (float)x;
        if (points64) points64[o + c] = x;
    }
    if (face_index) face_index[(long)b * num + i] = f;

    double c[3];
    double ln = 0.0;
    if (normals || COLOR == COLOR_TEXTURE) ln = cross_norm(t, c);
    if (normals) {                                           // preprocess.face_normals: n / max(|n|, 1e-300), zero where |n| = 0
        const double d = ln > 1e-300 ? ln : 1e-300;
#pragma unroll
        for (int k = 0; k < 3; ++k) normals[o + k] = ln > 0.0 ? (float)(c[k] / d) : 0.f;
    }
    if (COLOR == COLOR_GREY) {
#pragma unroll
        for (int k = 0; k < 3; ++k) colors[o + k] = 0.5f;
    } else if (COLOR == COLOR_VERTEX) {
        const int i0 = faces[(long)f * 3], i1 = faces[(long)f * 3 + 1], i2 = faces[(long)f * 3 + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double c0 = (double)vertex_colors[(long)i0 * color_channels + k] / 255.0;
            const double c1 = (double)vertex_colors[(long)i1 * color_channels + k] / 255.0;
            const double c2 = (double)vertex_colors[(long)i2 * color_channels + k] / 255.0;
            colors[o + k] = (float)(((c0 + c1) + c2) / 3.0);
        }
    } else if (COLOR == COLOR_TEXTURE) {
        const int idx[3] = {faces[(long)f * 3], faces[(long)f * 3 + 1], faces[(long)f * 3 + 2]};
        double wgt[3] = {(1.0 - r0) - r1, r0, r1};
        if (ln == 0.0) wgt[0] = wgt[1] = wgt[2] = 1.0 / 3.0; // the reference's rule for a triangle without area
        double s[2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
            s[a] = (wgt[0] * mod_one(uv[(long)idx[0] * 2 + a]) + wgt[1] * mod_one(uv[(long)idx[1] * 2 + a])) +
                   wgt[2] * mod_one(uv[(long)idx[2] * 2 + a]);
        const int col = clip_index(s[0] * (double)tex_w, tex_w);
        const int rw = clip_index((1.0 - s[1]) * (double)tex_h, tex_h);
        const unsigned char* px = texels + ((long)rw * tex_w + col) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) colors[o + k] = __fdiv_rn((float)px[k], 255.0f);
    }
}

// ------------------------------------------------------------------------------------------------ tracked samples
// The draw of surface_sample_kernel for sample i of an item, restated for the kernels that follow a sample through a clip: the
// same hash, the same bounded search of the frame-0 CDF row, the same reflection of the barycentric pair.
__device__ __forceinline__ int draw_sample(const double* __restrict__ row, int n_faces, unsigned long long seed_face,
                                           unsigned long long seed_bary, int i, double& r0, double& r1) {
    const double target = stream_uniform(seed_face, (unsigned long long)i) * row[n_faces - 1];
    int lo = 0, hi = n_faces;
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const int mid = lo + ((hi - lo) >> 1);
        if (row[mid] > target) hi = mid; else lo = mid + 1;
    }
    r0 = stream_uniform(seed_bary, 2ULL * (unsigned long long)i);
    r1 = stream_uniform(seed_bary, 2ULL * (unsigned long long)i + 1ULL);
    if (r0 + r1 > 1.0) {
        r0 = 1.0 - r0;
        r1 = 1.0 - r1;
    }
    return min(max(lo, 0), n_faces - 1);
}

__device__ __forceinline__ double norm3(const double (&a)[3]) { return __dsqrt_rn((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }
__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// np.clip(x, -1, 1): a NaN stays a NaN
__device__ __forceinline__ double clip_unit(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }

constexpr int NORMAL_THREADS = 256;                      // (frame, vertex) pairs per workgroup of vertex_normals_kernel
constexpr double PI = 3.141592653589793;                 // np.pi

// One lane = one vertex of one frame: it walks the vertex's corners in ascending order and adds each face's weighted unit normal
// to a running sum of its own -- a gather, so the order of the additions is the table's and nothing depends on scheduling.  A
// vertex of valence k recomputes k cross products (each face is visited by its three vertices); no per-face buffer, no
// per-vertex buffer, any valence.  Entries of the table outside their range are skipped, so a bad table reads nothing out of bounds.
template <int WEIGHTING>
__global__ __launch_bounds__(NORMAL_THREADS) void vertex_normals_kernel(const double* __restrict__ vertices, long stride_t, int n_vertices,
                                                                        const int* __restrict__ faces, int n_faces,
                                                                        const int* __restrict__ corner_offsets,
                                                                        const int* __restrict__ corner_list, long total,
                                                                        double* __restrict__ out) {
    const long g = (long)blockIdx.x * NORMAL_THREADS + threadIdx.x;
    if (g >= total) return;
    const int t = (int)(g / n_vertices);
    const int vtx = (int)(g % n_vertices);
    const double* v = vertices + (long)t * stride_t;
    const long n_corners = 3L * n_faces;
    const long lo = max(corner_offsets[vtx], 0);
    const long hi = min((long)corner_offsets[vtx + 1], n_corners);
    double n[3] = {0.0, 0.0, 0.0};
    for (long at = lo; at < hi; ++at) {
        const int corner = corner_list[at];
        if (corner < 0 || corner >= n_corners) continue;
        const int f = corner / 3, k = corner - 3 * f;
        const Tri tri = load_tri(v, faces, f);
        double c[3];
        const double ln = cross_norm(tri, c);
        if (!(ln != 0.0)) continue;                          // a face without area contributes nothing
        double w;
        if (WEIGHTING == M324_NORMALS_AREA) {
            w = 0.5 * ln;
        } else {
            const double l1 = norm3(tri.e1), l2 = norm3(tri.e2);
            double u[3], q[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) u[a] = tri.e1[a] / l1;
            double a0 = 0.0, a1 = 0.0;
            if (k != 1) {
#pragma unroll
                for (int a = 0; a < 3; ++a) q[a] = tri.e2[a] / l2;
                a0 = acos(clip_unit(dot3(u, q)));
            }
            if (k != 0) {
                const long i1 = faces[(long)f * 3 + 1], i2 = faces[(long)f * 3 + 2];
                double e3[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) e3[a] = v[i2 * 3 + a] - v[i1 * 3 + a];   // v2 - v1 itself: e2 - e1 rounds differently
                const double l3 = norm3(e3);
#pragma unroll
                for (int a = 0; a < 3; ++a) q[a] = e3[a] / l3;
                a1 = acos(clip_unit(-dot3(u, q)));
            }
            w = k == 0 ? a0 : (k == 1 ? a1 : (PI - a0) - a1);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) n[a] = n[a] + w * (c[a] / ln);
    }
    const double len = norm3(n);
    double* o = out + g * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = len != 0.0 ? n[a] / len : 0.0;
}

// One work item = (batch item, group of `frames_per_group` frames, tile of SAMPLE_THREADS samples) of a flat grid, one sample per
// lane.  The lane draws its face and weights once (draw_sample), keeps the three vertex indices and walks its frames; every
// (sample, frame) output is a function of the inputs alone, so the grouping -- chosen on the host to fill the chip -- never
// shows in the results.  Group 0 writes what has no frame axis (face index, colour).
__global__ __launch_bounds__(SAMPLE_THREADS) void surface_track_kernel(
    const double* __restrict__ vertices, long stride_b, long stride_t, const int* __restrict__ faces, int n_faces,
    const double* __restrict__ cdf, const unsigned long long* __restrict__ seeds, int num, int frames, int frames_per_group, int groups,
    int tiles, float* __restrict__ points, double* __restrict__ points64, int* __restrict__ face_index,
    const double* __restrict__ vertex_normals, long normal_stride_b, long normal_stride_t, float* __restrict__ normals,
    const double* __restrict__ face_uvs, const unsigned char* __restrict__ texels, int tex_h, int tex_w, float* __restrict__ colors) {
    const int tile = blockIdx.x % tiles;
    const int group = (blockIdx.x / tiles) % groups;
    const int b = blockIdx.x / (tiles * groups);
    const int i = tile * SAMPLE_THREADS + threadIdx.x;
    if (i >= num) return;
    double r0, r1;
    const int f = draw_sample(cdf + (long)b * n_faces, n_faces, seeds[(long)b * 2], seeds[(long)b * 2 + 1], i, r0, r1);
    const long i0 = faces[(long)f * 3], i1 = faces[(long)f * 3 + 1], i2 = faces[(long)f * 3 + 2];
    const double w0 = (1.0 - r0) - r1;

    if (group == 0) {
        if (face_index) face_index[(long)b * num + i] = f;
        if (colors) {
            const double* uv = face_uvs + (long)f * 6;
            const double s = (w0 * uv[0] + r0 * uv[2]) + r1 * uv[4];
            const double t = (w0 * uv[1] + r0 * uv[3]) + r1 * uv[5];
            const int col = clip_index(s * (double)(tex_w - 1), tex_w);
            const int rw = clip_index((1.0 - t) * (double)(tex_h - 1), tex_h);
            const unsigned char* px = texels + ((long)rw * tex_w + col) * 3;
            float* o = colors + ((long)b * num + i) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = (float)((double)px[k] / 255.0);
        }
    }

    const int t_end = min(frames, (group + 1) * frames_per_group);
    for (int t = group * frames_per_group; t < t_end; ++t) {
        const double* v = vertices + (long)b * stride_b + (long)t * stride_t;
        const long o = (((long)b * frames + t) * num + i) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v0 = v[i0 * 3 + c];
            const double e1 = v[i1 * 3 + c] - v0, e2 = v[i2 * 3 + c] - v0;
            const double x = (v0 + r0 * e1) + r1 * e2;
            points[o + c] = (float)x;
            if (points64) points64[o + c] = x;
        }
        if (normals) {
            const double* vn = vertex_normals + (long)b * normal_stride_b + (long)t * normal_stride_t;
            double m[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] = (w0 * vn[i0 * 3 + c] + r0 * vn[i1 * 3 + c]) + r1 * vn[i2 * 3 + c];
            const double len = norm3(m);
#pragma unroll
            for (int c = 0; c < 3; ++c) normals[o + c] = (float)(len == 0.0 ? m[c] : m[c] / len);
        }
    }
}

}  // namespace

extern "C" int m324_surface_plan(int n_faces, int batch, long* scratch_bytes) {
    M324_REQUIRE(n_faces > 0 && batch > 0, "m324_surface_plan: sizes must be positive (n_faces=%d batch=%d)", n_faces, batch);
    const int n_blocks = ceil_div(n_faces, SCAN_BLOCK);
    M324_REQUIRE((long)batch * n_blocks < 2147483647L, "m324_surface_plan: batch * face blocks too large");
    if (scratch_bytes) *scratch_bytes = n_blocks > 1 ? (long)batch * n_blocks * 8 : 0;
    return n_blocks;
}

extern "C" int m324_surface_cdf(const double* vertices, long stride_v, int n_vertices, const int* faces, int n_faces, int batch,
                                double* cdf, void* scratch, long scratch_bytes, void* stream) {
    M324_REQUIRE(vertices && faces && cdf, "m324_surface_cdf: null vertices, faces or cdf");
    M324_REQUIRE(n_vertices > 0 && n_faces > 0 && batch > 0 && stride_v >= 0,
                 "m324_surface_cdf: sizes must be positive (n_vertices=%d n_faces=%d batch=%d stride_v=%ld)", n_vertices, n_faces, batch, stride_v);
    long need = 0;
    const int n_blocks = m324_surface_plan(n_faces, batch, &need);
    if (n_blocks < 0) return n_blocks;
    M324_REQUIRE(need == 0 || (scratch && scratch_bytes >= need), "m324_surface_cdf: %d face blocks need %ld scratch bytes, got %ld", n_blocks, need,
                 scratch ? scratch_bytes : 0L);
    hipStream_t st = (hipStream_t)stream;
    double* totals = n_blocks > 1 ? (double*)scratch : nullptr;
    hipLaunchKernelGGL(surface_block_kernel, dim3(batch * n_blocks), dim3(SCAN_THREADS), 0, st, vertices, stride_v, faces, n_faces, n_blocks, cdf,
                       totals);
    if (n_blocks > 1)
        hipLaunchKernelGGL(surface_offset_kernel, dim3(batch * (n_blocks - 1)), dim3(SCAN_THREADS), 0, st, totals, n_faces, n_blocks, cdf);
    M324_CHECK_LAUNCH("m324_surface_cdf");
    return M324_OK;
}

extern "C" int m324_surface_sample(const double* vertices, long stride_v, int n_vertices, const int* faces, int n_faces, const double* cdf,
                                   const unsigned long long* seeds, int num, int batch, float* points, double* points64, int* face_index,
                                   float* normals, float* colors, const unsigned char* vertex_colors, int color_channels, const double* uv,
                                   const unsigned char* texels, int tex_h, int tex_w, void* stream) {
    M324_REQUIRE(vertices && faces && cdf && seeds && points, "m324_surface_sample: null vertices, faces, cdf, seeds or points");
    M324_REQUIRE(n_vertices > 0 && n_faces > 0 && num > 0 && batch > 0 && stride_v >= 0,
                 "m324_surface_sample: sizes must be positive (n_vertices=%d n_faces=%d num=%d batch=%d stride_v=%ld)", n_vertices, n_faces, num,
                 batch, stride_v);
    const int tiles = ceil_div(num, SAMPLE_THREADS);
    M324_REQUIRE((long)batch * tiles < 2147483647L, "m324_surface_sample: batch * sample tiles too large");
    int color = COLOR_NONE;
    if (colors) {
        if (vertex_colors) {
            M324_REQUIRE(color_channels == 3 || color_channels == 4, "m324_surface_sample: vertex colours have 3 or 4 channels, got %d", color_channels);
            color = COLOR_VERTEX;
        } else if (uv || texels) {
            M324_REQUIRE(uv && texels && tex_h > 0 && tex_w > 0, "m324_surface_sample: a texture needs uv, texels and a positive size (%d x %d)", tex_h,
                         tex_w);
            color = COLOR_TEXTURE;
        } else {
            color = COLOR_GREY;
        }
    }
    const dim3 grid(batch * tiles), block(SAMPLE_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define SURFACE_LAUNCH(MODE)                                                                                                          \
    hipLaunchKernelGGL(surface_sample_kernel<MODE>, grid, block, 0, st, vertices, stride_v, faces, n_faces, cdf, seeds, num, tiles, points, \
                       points64, face_index, normals, colors, vertex_colors, color_channels, uv, texels, tex_h, tex_w)
    switch (color) {
        case COLOR_VERTEX: SURFACE_LAUNCH(COLOR_VERTEX); break;
        case COLOR_TEXTURE: SURFACE_LAUNCH(COLOR_TEXTURE); break;
        case COLOR_GREY: SURFACE_LAUNCH(COLOR_GREY); break;
        default: SURFACE_LAUNCH(COLOR_NONE); break;
    }
#undef SURFACE_LAUNCH
    M324_CHECK_LAUNCH("m324_surface_sample");
    return M324_OK;
}

extern "C" int m324_vertex_normals(const double* vertices, long stride_t, int n_vertices, const int* faces, int n_faces,
                                   const int* corner_offsets, const int* corner_list, int frames, int weighting, double* out, void* stream) {
    M324_REQUIRE(vertices && faces && corner_offsets && corner_list && out,
                 "m324_vertex_normals: null vertices, faces, corner_offsets, corner_list or out");
    M324_REQUIRE(n_vertices > 0 && n_faces > 0 && frames > 0 && stride_t >= 0 && n_faces <= 2147483647 / 3,
                 "m324_vertex_normals: sizes must be positive (n_vertices=%d n_faces=%d frames=%d stride_t=%ld)", n_vertices, n_faces, frames, stride_t);
    M324_REQUIRE(weighting == M324_NORMALS_ANGLE || weighting == M324_NORMALS_AREA, "m324_vertex_normals: weighting must be %d (angle) or %d (area), got %d",
                 M324_NORMALS_ANGLE, M324_NORMALS_AREA, weighting);
    const long total = (long)frames * n_vertices;
    M324_REQUIRE((total + NORMAL_THREADS - 1) / NORMAL_THREADS < 2147483647L, "m324_vertex_normals: frames * n_vertices too large");
    const dim3 grid(ceil_div(total, NORMAL_THREADS)), block(NORMAL_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (weighting == M324_NORMALS_AREA)
        hipLaunchKernelGGL(vertex_normals_kernel<M324_NORMALS_AREA>, grid, block, 0, st, vertices, stride_t, n_vertices, faces, n_faces, corner_offsets,
                           corner_list, total, out);
    else
        hipLaunchKernelGGL(vertex_normals_kernel<M324_NORMALS_ANGLE>, grid, block, 0, st, vertices, stride_t, n_vertices, faces, n_faces, corner_offsets,
                           corner_list, total, out);
    M324_CHECK_LAUNCH("m324_vertex_normals");
    return M324_OK;
}

extern "C" int m324_surface_track(const double* vertices, long stride_b, long stride_t, int n_vertices, const int* faces, int n_faces,
                                  const double* cdf, const unsigned long long* seeds, int num, int batch, int frames, float* points,
                                  double* points64, int* face_index, const double* vertex_normals, long normal_stride_b, long normal_stride_t,
                                  float* normals, const double* face_uvs, const unsigned char* texels, int tex_h, int tex_w, float* colors,
                                  void* stream) {
    M324_REQUIRE(vertices && faces && cdf && seeds && points, "m324_surface_track: null vertices, faces, cdf, seeds or points");
    M324_REQUIRE(n_vertices > 0 && n_faces > 0 && num > 0 && batch > 0 && frames > 0 && stride_b >= 0 && stride_t >= 0,
                 "m324_surface_track: sizes must be positive (n_vertices=%d n_faces=%d num=%d batch=%d frames=%d stride_b=%ld stride_t=%ld)", n_vertices,
                 n_faces, num, batch, frames, stride_b, stride_t);
    M324_REQUIRE(!normals == !vertex_normals && normal_stride_b >= 0 && normal_stride_t >= 0,
                 "m324_surface_track: normals and vertex_normals go together, with non-negative strides (%ld, %ld)", normal_stride_b, normal_stride_t);
    M324_REQUIRE(colors ? (face_uvs && texels && tex_h > 0 && tex_w > 0) : (!face_uvs && !texels),
                 "m324_surface_track: colors, face_uvs and texels of a positive size (%d x %d) go together", tex_h, tex_w);
    const int tiles = ceil_div(num, SAMPLE_THREADS);
    // frames per lane: as many as still leave four workgroups per compute unit, so a single long clip spreads over the chip and a
    // large batch amortises the draw.  The results do not depend on it.
    const long items = (long)batch * tiles * frames;
    long per = items / (4L * m324::cu_count());
    per = per < 1 ? 1 : (per > frames ? frames : per);
    const int groups = ceil_div(frames, per);
    M324_REQUIRE((long)batch * tiles * groups < 2147483647L, "m324_surface_track: batch * frame groups * sample tiles too large");
    hipLaunchKernelGGL(surface_track_kernel, dim3(batch * groups * tiles), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, vertices, stride_b, stride_t,
                       faces, n_faces, cdf, seeds, num, frames, (int)per, groups, tiles, points, points64, face_index, vertex_normals, normal_stride_b,
                       normal_stride_t, normals, face_uvs, texels, tex_h, tex_w, colors);
    M324_CHECK_LAUNCH("m324_surface_track");
    return M324_OK;
}
