// Mesh clip voxeliser (gfx950): exact surface occupancy of every frame of a clip with one topology in a bit grid, the
// orthographic fill of such a grid and the popcounts behind a volumetric IoU -- the 3-D sibling of csrc/render.hip.
// replaces: compute_iou_voxel of the reference's evaluation/evaluation_pcd.py:612-637 (trimesh on the CPU there, and commented out).
//
// The arithmetic IS the contract (include/m324.h spells it out and the test model is written from there): vertices are snapped to
// 1/16 voxel, a triangle marks a voxel iff none of the 13 axes of the triangle / closed-cube separating-axis test separates them,
// evaluated in int64, and marking is a 32-bit atomic OR, which is idempotent and commutes.  So no output depends on arrival
// order, grid shape, CU count, queue order or big_voxels.  The counts are integer sums; the quotient is formed on the host.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr long ALIGN = 256;                              // every scratch region starts on a 256-byte boundary

// Regions of the scratch buffer, in this order: queue counter, snapped vertices, queue.
struct Layout {
    long counter, snap, queue, total;
};

inline long round_up(long v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }

inline Layout layout_of(int n_vertices, int n_faces, int frames) {
    Layout l;
    l.counter = 0;
    l.snap = ALIGN;
    l.queue = l.snap + round_up((long)frames * n_vertices * 16);
    l.total = l.queue + round_up((long)frames * n_faces * 4);
    return l;
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }   // false for a NaN as well

// One lane = one (frame, vertex).  snap[g] = (q_x, q_y, q_z, valid); a valid vertex outside [0, 16 G]^3 counts in outside[frame].
__global__ __launch_bounds__(THREADS) void voxel_snap_kernel(const float* __restrict__ vertices, long stride_t, int n_vertices, long total,
                                                             float half, float scale, int limit, int4* __restrict__ snap,
                                                             int* __restrict__ outside) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= total) return;
    const long t = g / n_vertices, v = g % n_vertices;
    const float* src = vertices + t * stride_t + v * 3;
    const float x = src[0], y = src[1], z = src[2];
    int4 q = make_int4(0, 0, 0, 0);
    if (finitef(x) && finitef(y) && finitef(z)) {
        q.x = (int)rintf(clampf((x + half) * scale, -131072.f, 131072.f));
        q.y = (int)rintf(clampf((y + half) * scale, -131072.f, 131072.f));
        q.z = (int)rintf(clampf((z + half) * scale, -131072.f, 131072.f));
        q.w = 1;
        if (q.x < 0 || q.x > limit || q.y < 0 || q.y > limit || q.z < 0 || q.z > limit) atomicAdd(outside + t, 1);
    }
    snap[g] = q;
}

// The integer form of one triangle.  Edge axis 3 m + u is a = e_m x u; with c1 = (u + 1) mod 3 and c2 = (u + 2) mod 3 its only
// non-zero components are a_c1 = e_m[c2] and a_c2 = -e_m[c1], so a . p = e_m[c2] * p_c1 - e_m[c1] * p_c2.
struct Tri {
    long long n[3];                                      // e_0 x e_1
    long long nd, nr;                                    // n . v_0 and 8 (|n_x| + |n_y| + |n_z|)
    int e[3][3];                                         // the edges
    long long lo[9], hi[9];                              // min and max over the vertices of a . v_l
    long long r[9];                                      // 8 (|a_x| + |a_y| + |a_z|)
    int i0, i1, j0, j1, k0, k1;                          // voxels whose closed cube meets the bounding box, clipped to the grid (inclusive)
};

// 64-bit helpers spelled out: no overload set decides how wide min, max and abs are
__device__ __forceinline__ long long abs64(long long v) { return v < 0 ? -v : v; }
__device__ __forceinline__ long long min64(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long max64(long long a, long long b) { return a > b ? a : b; }

// false: nothing to mark (an index out of range, an invalid vertex, or a bounding box that misses the grid)
__device__ __forceinline__ bool setup_tri(const int* __restrict__ faces, long f, int n_vertices, const int4* __restrict__ snap, int side, Tri& t) {
    const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)n_vertices || (unsigned)i1 >= (unsigned)n_vertices || (unsigned)i2 >= (unsigned)n_vertices) return false;
    const int4 q[3] = {snap[i0], snap[i1], snap[i2]};
    if (!(q[0].w & q[1].w & q[2].w)) return false;
    const int v[3][3] = {{q[0].x, q[0].y, q[0].z}, {q[1].x, q[1].y, q[1].z}, {q[2].x, q[2].y, q[2].z}};
    int lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        t.e[0][c] = v[1][c] - v[0][c];
        t.e[1][c] = v[2][c] - v[1][c];
        t.e[2][c] = v[0][c] - v[2][c];
        lo[c] = min(v[0][c], min(v[1][c], v[2][c]));
        hi[c] = max(v[0][c], max(v[1][c], v[2][c]));
    }
    // The three cube axes: voxel i along an axis passes iff 16 i + 16 >= min and 16 i <= max.  That is exactly the box below, so the
    // walks never test them again (arithmetic shifts: floor).
    t.i0 = max((lo[0] - 1) >> 4, 0);
    t.i1 = min(hi[0] >> 4, side - 1);
    t.j0 = max((lo[1] - 1) >> 4, 0);
    t.j1 = min(hi[1] >> 4, side - 1);
    t.k0 = max((lo[2] - 1) >> 4, 0);
    t.k1 = min(hi[2] >> 4, side - 1);
    if (t.i0 > t.i1 || t.j0 > t.j1 || t.k0 > t.k1) return false;
    t.n[0] = (long long)t.e[0][1] * t.e[1][2] - (long long)t.e[0][2] * t.e[1][1];
    t.n[1] = (long long)t.e[0][2] * t.e[1][0] - (long long)t.e[0][0] * t.e[1][2];
    t.n[2] = (long long)t.e[0][0] * t.e[1][1] - (long long)t.e[0][1] * t.e[1][0];
    t.nd = t.n[0] * v[0][0] + t.n[1] * v[0][1] + t.n[2] * v[0][2];
    t.nr = 8 * (abs64(t.n[0]) + abs64(t.n[1]) + abs64(t.n[2]));
#pragma unroll
    for (int m = 0; m < 3; ++m) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int c1 = (u + 1) % 3, c2 = (u + 2) % 3;
            const long long p0 = (long long)t.e[m][c2] * v[0][c1] - (long long)t.e[m][c1] * v[0][c2];
            const long long p1 = (long long)t.e[m][c2] * v[1][c1] - (long long)t.e[m][c1] * v[1][c2];
            const long long p2 = (long long)t.e[m][c2] * v[2][c1] - (long long)t.e[m][c1] * v[2][c2];
            t.lo[m * 3 + u] = min64(p0, min64(p1, p2));
            t.hi[m * 3 + u] = max64(p0, max64(p1, p2));
            t.r[m * 3 + u] = 8 * (abs64(t.e[m][c2]) + abs64(t.e[m][c1]));
        }
    }
    return true;
}

// The ten axes the box does not already decide, for the voxel whose centre is c (sub-voxel units): a . v'_l = a . v_l - a . c.
__device__ __forceinline__ bool overlaps(const Tri& t, int cx, int cy, int cz) {
    const long long c[3] = {cx, cy, cz};
    if (abs64(t.nd - (t.n[0] * c[0] + t.n[1] * c[1] + t.n[2] * c[2])) > t.nr) return false;
    bool hit = true;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int c1 = (u + 1) % 3, c2 = (u + 2) % 3, ax = m * 3 + u;
            const long long s = t.e[m][c2] * c[c1] - t.e[m][c1] * c[c2];
            hit = hit && !(t.lo[ax] - s > t.r[ax] || t.hi[ax] - s < -t.r[ax]);
        }
    }
    return hit;
}

// Word w of row (j, k) of one frame: the voxels of the triangle's box inside it are tested, their bits leave in one atomic OR.
// (j, k, w) lie inside the grid because the box is clipped to it.
__device__ __forceinline__ void mark_word(const Tri& t, int j, int k, int w, int side, unsigned* __restrict__ grid) {
    const int first = max(t.i0, 32 * w), last = min(t.i1, 32 * w + 31);
    unsigned mask = 0;
    for (int i = first; i <= last; ++i)
        if (overlaps(t, 16 * i + 8, 16 * j + 8, 16 * k + 8)) mask |= 1u << (i & 31);
    // the result is not used: a no-return atomic
    if (mask) __hip_atomic_fetch_or(grid + ((long)k * side + j) * (side >> 5) + w, mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane = one (frame, face).  A triangle whose box holds at most big_voxels voxels is walked by its lane; the others go to the
// queue: one counter add per wave for all its lanes that queue (the ballot is taken where the whole wave has reconverged).
__global__ __launch_bounds__(THREADS) void voxel_small_kernel(const int* __restrict__ faces, int n_faces, int n_vertices, long total, int side,
                                                              int big_voxels, const int4* __restrict__ snap, unsigned* __restrict__ grid,
                                                              unsigned* __restrict__ counter, unsigned* __restrict__ queue) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    bool queued = false;
    if (g < total) {
        const long frame = g / n_faces, f = g % n_faces;
        Tri t;
        if (setup_tri(faces, f, n_vertices, snap + frame * n_vertices, side, t)) {
            const long box = (long)(t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) * (t.k1 - t.k0 + 1);
            if (box > big_voxels) {
                queued = true;
            } else {
                unsigned* gf = grid + frame * side * side * (side >> 5);
                for (int k = t.k0; k <= t.k1; ++k)
                    for (int j = t.j0; j <= t.j1; ++j)
                        for (int w = t.i0 >> 5; w <= t.i1 >> 5; ++w) mark_word(t, j, k, w, side, gf);
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

// One workgroup = one queue entry at a time (a grid-stride walk over the entries the first pass left), lanes striding over the
// (word, j, k) triples of the box.
__global__ __launch_bounds__(THREADS) void voxel_queue_kernel(const int* __restrict__ faces, int n_faces, int n_vertices, long total, int side,
                                                              const int4* __restrict__ snap, unsigned* __restrict__ grid,
                                                              const unsigned* __restrict__ counter, const unsigned* __restrict__ queue) {
    const long count = min64((long)*counter, total);
    for (long e = blockIdx.x; e < count; e += gridDim.x) {
        const long g = queue[e];
        if (g >= total) continue;
        const long frame = g / n_faces, f = g % n_faces;
        Tri t;
        if (!setup_tri(faces, f, n_vertices, snap + frame * n_vertices, side, t)) continue;
        unsigned* gf = grid + frame * side * side * (side >> 5);
        const int w0 = t.i0 >> 5, nw = (t.i1 >> 5) - w0 + 1, nj = t.j1 - t.j0 + 1;
        const long n = (long)nw * nj * (t.k1 - t.k0 + 1);
        for (long i = threadIdx.x; i < n; i += THREADS) {
            const long row = i / nw;
            mark_word(t, t.j0 + (int)(row % nj), t.k0 + (int)(row / nj), w0 + (int)(i % nw), side, gf);
        }
    }
}

// ---- orthographic fill: acc = E_z, then acc &= E_y, then acc &= E_x, each read from the untouched surface grid -----------------
// One lane = one column of words along z, (frame, j, w): a forward OR scan leaves the prefix in acc, a backward one ANDs the suffix in.
__global__ __launch_bounds__(THREADS) void voxel_fill_z_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ acc, long total, int side) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= total) return;
    const long slab = (long)side * (side >> 5);          // words of one z layer; g = frame * slab + (j * W + w)
    const long at = (g / slab) * slab * side + g % slab;
    unsigned run = 0;
    for (int k = 0; k < side; ++k) {
        run |= src[at + k * slab];
        acc[at + k * slab] = run;
    }
    run = 0;
    for (int k = side - 1; k >= 0; --k) {
        run |= src[at + k * slab];
        acc[at + k * slab] &= run;
    }
}

// One lane = one column of words along y, (frame, k, w).
__global__ __launch_bounds__(THREADS) void voxel_fill_y_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ acc, long total, int side) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= total) return;
    const int W = side >> 5;
    const long at = (g / W) * W * side + g % W;           // g = (frame * side + k) * W + w
    unsigned run = 0;
    for (int j = 0; j < side; ++j) {
        run |= src[at + (long)j * W];
        acc[at + (long)j * W] &= run;
    }
    run = 0;
    for (int j = side - 1; j >= 0; --j) {
        run |= src[at + (long)j * W];
        acc[at + (long)j * W] &= run;
    }
}

// One lane = one row of words along x, (frame, k, j): the bits from the row's first occupied voxel to its last.
__global__ __launch_bounds__(THREADS) void voxel_fill_x_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ acc, long total, int side) {
    const long g = (long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= total) return;
    const int W = side >> 5;
    const unsigned* row = src + g * W;
    int first = side, last = -1;
    for (int w = 0; w < W; ++w) {
        const unsigned v = row[w];
        if (v) {
            if (first == side) first = 32 * w + (__ffs((int)v) - 1);
            last = 32 * w + 31 - __clz((int)v);
        }
    }
    for (int w = 0; w < W; ++w) {
        const int a = max(first - 32 * w, 0), b = min(last - 32 * w, 31);
        const unsigned mask = (a > 31 || b < 0) ? 0u : ((0xffffffffu >> (31 - b)) & (0xffffffffu << a));
        acc[g * W + w] &= mask;
    }
}

// ---- counts: blockIdx.y = frame; a workgroup strides over the frame's 16-byte chunks, reduces, and adds three integers -----------
__global__ __launch_bounds__(THREADS) void voxel_counts_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, long chunks,
                                                               unsigned long long* __restrict__ counts) {
    const uint4* fa = a + blockIdx.y * chunks;
    const uint4* fb = b + blockIdx.y * chunks;
    unsigned na = 0, nb = 0, nab = 0;                    // a frame holds at most 2^30 voxels: no sum below overflows 32 bits
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < chunks; i += (long)gridDim.x * THREADS) {
        const uint4 x = fa[i], y = fb[i];
        na += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
        nb += __popc(y.x) + __popc(y.y) + __popc(y.z) + __popc(y.w);
        nab += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        na += __shfl_xor(na, s, 64);
        nb += __shfl_xor(nb, s, 64);
        nab += __shfl_xor(nab, s, 64);
    }
    __shared__ unsigned part[THREADS / 64][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = na;
        part[wave][1] = nb;
        part[wave][2] = nab;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned sum = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) sum += part[w][threadIdx.x];
        if (sum) atomicAdd(counts + blockIdx.y * 3 + threadIdx.x, (unsigned long long)sum);
    }
}

// Everything the entry points share: sizes first (no HIP call before they pass).
int check_side(const char* who, int side) {
    M324_REQUIRE(side >= M324_VOXEL_MIN_SIDE && side <= M324_VOXEL_MAX_SIDE && side % 32 == 0,
                 "%s: the grid side must be a multiple of 32 in %d..%d, got %d", who, M324_VOXEL_MIN_SIDE, M324_VOXEL_MAX_SIDE, side);
    return M324_OK;
}

int check_sizes(const char* who, int n_vertices, int n_faces, int frames, int resolution, int half) {
    M324_REQUIRE(resolution >= 16 && resolution % 16 == 0, "%s: resolution must be a positive multiple of 16, got %d", who, resolution);
    M324_REQUIRE(half >= 1 && half <= M324_VOXEL_MAX_SIDE && 2L * half * resolution >= M324_VOXEL_MIN_SIDE && 2L * half * resolution <= M324_VOXEL_MAX_SIDE,
                 "%s: the grid side 2 * half * resolution must be in %d..%d (half=%d resolution=%d)", who, M324_VOXEL_MIN_SIDE,
                 M324_VOXEL_MAX_SIDE, half, resolution);
    M324_REQUIRE(frames >= 1 && n_vertices >= 1 && n_faces >= 0, "%s: need frames >= 1, n_vertices >= 1, n_faces >= 0 (frames=%d n_vertices=%d n_faces=%d)",
                 who, frames, n_vertices, n_faces);
    M324_REQUIRE((long)frames * n_faces < 2147483647L && (long)frames * n_vertices < 2147483647L,
                 "%s: frames * n_faces and frames * n_vertices must stay below 2^31 (frames=%d n_vertices=%d n_faces=%d): voxelise fewer frames per call",
                 who, frames, n_vertices, n_faces);
    return M324_OK;
}

inline long grid_bytes(int frames, int side) { return (long)frames * side * side * (side >> 5) * 4; }

}  // namespace

extern "C" int m324_voxel_plan(int n_vertices, int n_faces, int frames, int resolution, int half, long* scratch_bytes) {
    const int rc = check_sizes("m324_voxel_plan", n_vertices, n_faces, frames, resolution, half);
    if (rc != M324_OK) return rc;
    if (scratch_bytes) *scratch_bytes = layout_of(n_vertices, n_faces, frames).total;
    return M324_OK;
}

extern "C" int m324_voxelize(const float* vertices, long stride_t, int n_vertices, const int* faces, int n_faces, int frames, int resolution,
                             int half, int big_voxels, int* grid, int* outside, void* scratch, long scratch_bytes, void* stream) {
    M324_REQUIRE(vertices && grid && outside && scratch && (faces || n_faces == 0), "m324_voxelize: null vertices, faces, grid, outside or scratch");
    const int rc = check_sizes("m324_voxelize", n_vertices, n_faces, frames, resolution, half);
    if (rc != M324_OK) return rc;
    M324_REQUIRE(stride_t >= 0, "m324_voxelize: stride_t must not be negative, got %ld", stride_t);
    M324_REQUIRE(big_voxels >= 0, "m324_voxelize: big_voxels must not be negative, got %d", big_voxels);
    const Layout l = layout_of(n_vertices, n_faces, frames);
    M324_REQUIRE(scratch_bytes >= l.total, "m324_voxelize: needs %ld scratch bytes (m324_voxel_plan), got %ld", l.total, scratch_bytes);
    M324_REQUIRE(((uintptr_t)scratch & 15) == 0 && ((uintptr_t)grid & 3) == 0 && ((uintptr_t)outside & 3) == 0,
                 "m324_voxelize: scratch must be 16-byte aligned, grid and outside 4-byte aligned");
    const int side = 2 * half * resolution;
    char* base = (char*)scratch;
    hipStream_t st = (hipStream_t)stream;
    unsigned* counter = (unsigned*)(base + l.counter);
    int4* snap = (int4*)(base + l.snap);
    unsigned* queue = (unsigned*)(base + l.queue);
    hipError_t e = hipMemsetAsync(grid, 0, (size_t)grid_bytes(frames, side), st);
    if (e == hipSuccess) e = hipMemsetAsync(outside, 0, (size_t)frames * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(counter, 0, ALIGN, st);
    if (e != hipSuccess) M324_FAIL(M324_ERR_HIP, "m324_voxelize: %s", hipGetErrorString(e));
    const long nv = (long)frames * n_vertices;
    hipLaunchKernelGGL(voxel_snap_kernel, dim3(ceil_div(nv, THREADS)), dim3(THREADS), 0, st, vertices, stride_t, n_vertices, nv, (float)half,
                       (float)(16 * resolution), 16 * side, snap, outside);
    const long total = (long)frames * n_faces;
    if (total > 0) {
        hipLaunchKernelGGL(voxel_small_kernel, dim3(ceil_div(total, THREADS)), dim3(THREADS), 0, st, faces, n_faces, n_vertices, total, side, big_voxels,
                           snap, (unsigned*)grid, counter, queue);
        // as many workgroups as the chip holds a few times over, never more than there can be entries
        const long chip = 16L * m324::cu_count();
        const long groups = total < chip ? total : chip;
        hipLaunchKernelGGL(voxel_queue_kernel, dim3((unsigned)groups), dim3(THREADS), 0, st, faces, n_faces, n_vertices, total, side, snap,
                           (unsigned*)grid, counter, queue);
    }
    M324_CHECK_LAUNCH("m324_voxelize");
    return M324_OK;
}

extern "C" int m324_voxel_fill(const int* grid, int* out, int frames, int side, void* scratch, long scratch_bytes, void* stream) {
    M324_REQUIRE(grid && out, "m324_voxel_fill: null grid or out");
    const int rc = check_side("m324_voxel_fill", side);
    if (rc != M324_OK) return rc;
    M324_REQUIRE(frames >= 1, "m324_voxel_fill: frames must be positive, got %d", frames);
    M324_REQUIRE(((uintptr_t)grid & 3) == 0 && ((uintptr_t)out & 3) == 0, "m324_voxel_fill: grid and out must be 4-byte aligned");
    const long bytes = grid_bytes(frames, side);
    const bool in_place = (const int*)out == grid;
    unsigned* acc = (unsigned*)out;
    if (in_place) {
        M324_REQUIRE(scratch && scratch_bytes >= bytes, "m324_voxel_fill: filling in place needs %ld scratch bytes (the grid's size), got %ld", bytes,
                     scratch ? scratch_bytes : 0L);
        M324_REQUIRE(((uintptr_t)scratch & 3) == 0, "m324_voxel_fill: scratch must be 4-byte aligned");
        acc = (unsigned*)scratch;
    } else {
        M324_REQUIRE((uintptr_t)out + bytes <= (uintptr_t)grid || (uintptr_t)grid + bytes <= (uintptr_t)out,
                     "m324_voxel_fill: out overlaps grid without being grid");
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned* src = (const unsigned*)grid;
    const long columns = (long)frames * side * (side >> 5), rows = (long)frames * side * side;
    hipLaunchKernelGGL(voxel_fill_z_kernel, dim3(ceil_div(columns, THREADS)), dim3(THREADS), 0, st, src, acc, columns, side);
    hipLaunchKernelGGL(voxel_fill_y_kernel, dim3(ceil_div(columns, THREADS)), dim3(THREADS), 0, st, src, acc, columns, side);
    hipLaunchKernelGGL(voxel_fill_x_kernel, dim3(ceil_div(rows, THREADS)), dim3(THREADS), 0, st, src, acc, rows, side);
    M324_CHECK_LAUNCH("m324_voxel_fill");
    if (in_place) {
        const hipError_t e = hipMemcpyAsync(out, acc, (size_t)bytes, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) M324_FAIL(M324_ERR_HIP, "m324_voxel_fill: %s", hipGetErrorString(e));
    }
    return M324_OK;
}

extern "C" int m324_voxel_counts(const int* a, const int* b, int frames, int side, long* counts, void* stream) {
    M324_REQUIRE(a && b && counts, "m324_voxel_counts: null a, b or counts");
    const int rc = check_side("m324_voxel_counts", side);
    if (rc != M324_OK) return rc;
    M324_REQUIRE(frames >= 1 && frames <= 65535, "m324_voxel_counts: frames must be in 1..65535, got %d", frames);
    M324_REQUIRE(((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0 && ((uintptr_t)counts & 7) == 0,
                 "m324_voxel_counts: a and b must be 16-byte aligned, counts 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)frames * 3 * 8, st);
    if (e != hipSuccess) M324_FAIL(M324_ERR_HIP, "m324_voxel_counts: %s", hipGetErrorString(e));
    const long chunks = (long)side * side * (side >> 5) / 4;                 // 16-byte chunks of a frame: side % 32 == 0 makes it whole
    const long want = (chunks + THREADS * 8 - 1) / (THREADS * 8);            // about eight chunks per lane
    const unsigned groups = (unsigned)(want < 1024 ? want : 1024);
    hipLaunchKernelGGL(voxel_counts_kernel, dim3(groups, (unsigned)frames), dim3(THREADS), 0, st, (const uint4*)a, (const uint4*)b, chunks,
                       (unsigned long long*)counts);
    M324_CHECK_LAUNCH("m324_voxel_counts");
    return M324_OK;
}
