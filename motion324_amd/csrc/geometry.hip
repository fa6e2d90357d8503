// Geometry evaluation kernels (gfx950): batched brute-force nearest neighbour, distance statistics, similarity transform of a
// point set and the moment sums of one ICP iteration -- what motion324_amd/evaluation.py (Chamfer distance, F-score, ICP
// alignment; evaluation/evaluation_pcd.py in the reference, cKDTree queries on the CPU there) runs on the device.
//
// Determinism: no atomics anywhere.  Every reduction is "per-workgroup partials in a fixed order, then one workgroup adds them
// in index order"; the sliced search writes per-slice (d2, index) partials and a second kernel takes their lexicographic
// minimum, so a result never depends on the slice count, the grid or the arrival order.
#include "common.h"
#include <math.h>

#ifndef M324_NN_QPL
#define M324_NN_QPL 4          // queries held in registers per lane (tools/eval_time.py builds a lab copy with 8; profiles/geometry_eval.md)
#endif

namespace {

constexpr int NN_THREADS = 256;
constexpr int NN_QPL = M324_NN_QPL;
constexpr int NN_TILE = NN_THREADS * NN_QPL;      // queries per work item
constexpr int NN_CHUNK = 1024;                    // reference records staged per LDS fill (16 KiB)
constexpr int NN_MIN_SLICE = 256;                 // an automatic slice is never shorter than this
constexpr int NN_MAX_SLICES = 64;

// One work item = (batch item, query tile, reference slice) of a flat grid.  Reference points are staged in LDS as 16-byte
// records (x, y, z, pad) and read back with one ds_read_b128 at a wave-uniform address (a broadcast: one LDS cycle per lane
// group, no bank conflict); each lane keeps NN_QPL queries in registers, so one LDS read feeds NN_QPL distance evaluations
// (7 or 9 VALU instructions each) and the loop is VALU-bound.  d2 = dx*dx + dy*dy + dz*dz from coordinate differences in fp32,
// evaluated as fma(dz, dz, fma(dy, dy, dx * dx)) everywhere, so every instantiation and every grid gives the same bits.
// WITH_INDEX = false: one v_min_f32 per pair; true: compare + two selects.  Strict `<` over ascending reference indices:
// the lowest index wins ties; a pair that does not compare below +inf (non-finite coordinates) never wins.
// FINAL = true (one slice): writes sqrt(d2) / index; false: writes the slice's partial (d2, index) into scratch.
template <bool WITH_INDEX, bool FINAL>
__global__ __launch_bounds__(NN_THREADS) void nn_search_kernel(const float* __restrict__ query, long stride_q, int nq,
                                                               const float* __restrict__ ref, long stride_r, int nr, int qtiles,
                                                               int slices, int per_slice, float* __restrict__ dist_out,
                                                               int* __restrict__ idx_out, float* __restrict__ part_d2,
                                                               int* __restrict__ part_idx, long part_stride) {
    __shared__ __attribute__((aligned(16))) float4 recs[NN_CHUNK];
    const int item = blockIdx.x;
    const int slice = item % slices;
    const int qt = (item / slices) % qtiles;
    const int b = item / (slices * qtiles);
    const float* q = query + (long)b * stride_q;
    const float* r = ref + (long)b * stride_r;
    const int tid = threadIdx.x;
    const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) unsigned char*)recs;

    float qx[NN_QPL], qy[NN_QPL], qz[NN_QPL], best[NN_QPL];
    int besti[NN_QPL];
#pragma unroll
    for (int k = 0; k < NN_QPL; ++k) {
        const int qi = qt * NN_TILE + k * NN_THREADS + tid;
        const bool live = qi < nq;
        qx[k] = live ? q[(long)qi * 3] : 0.f;
        qy[k] = live ? q[(long)qi * 3 + 1] : 0.f;
        qz[k] = live ? q[(long)qi * 3 + 2] : 0.f;
        best[k] = INFINITY;
        besti[k] = -1;
    }

    const int r_begin = slice * per_slice;
    const int r_end = min(nr, r_begin + per_slice);
    for (int r0 = r_begin; r0 < r_end; r0 += NN_CHUNK) {
        const int cnt = min(NN_CHUNK, r_end - r0);
        const int cnt4 = (cnt + 3) & ~3;                     // <= NN_CHUNK: NN_CHUNK is a multiple of 4
        __syncthreads();
        for (int e = tid; e < cnt4; e += NN_THREADS) {
            float4 v = make_float4(INFINITY, INFINITY, INFINITY, 0.f);      // pad records never win: d2 is +inf or NaN
            if (e < cnt) {
                const float* p = r + (long)(r0 + e) * 3;
                v = make_float4(p[0], p[1], p[2], 0.f);
            }
            recs[e] = v;
        }
        __syncthreads();
        for (int j = 0; j < cnt4; j += 4) {
            // four records per step, each ONE ds_read_b128 at a wave-uniform address.  Written out: from `recs[j]` the compiler
            // drops the unused pad component and emits ds_read_b96, which is banked like ds_read_b32 and moves half the bytes per
            // LDS cycle.  The wait sits inside the statement (the compiler does not count these reads); other waves of the CU
            // cover it -- the slicing rule asks for two work items per CU.
            f32x4 p[4];
            asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:32\n\t"
                         "ds_read_b128 %3, %4 offset:48\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(p[0]), "=&v"(p[1]), "=&v"(p[2]), "=&v"(p[3])
                         : "v"(lds0 + 16u * j)
                         : "memory");
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int k = 0; k < NN_QPL; ++k) {
                    const float dx = p[u].x - qx[k], dy = p[u].y - qy[k], dz = p[u].z - qz[k];
                    const float d = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));      // one fixed order in every instantiation
                    if (WITH_INDEX) {
                        const bool closer = d < best[k];
                        best[k] = closer ? d : best[k];
                        besti[k] = closer ? r0 + j + u : besti[k];
                    } else {
                        best[k] = fminf(best[k], d);            // a NaN d leaves best alone
                    }
                }
            }
        }
    }

#pragma unroll
    for (int k = 0; k < NN_QPL; ++k) {
        const int qi = qt * NN_TILE + k * NN_THREADS + tid;
        if (qi >= nq) continue;
        const long o = (long)b * nq + qi;
        if (FINAL) {
            if (dist_out) dist_out[o] = __fsqrt_rn(best[k]);
            if (WITH_INDEX) idx_out[o] = besti[k];
        } else {
            part_d2[(long)slice * part_stride + o] = best[k];
            if (WITH_INDEX) part_idx[(long)slice * part_stride + o] = besti[k];
        }
    }
}

// Lexicographic minimum (d2, index) over the slices of one (batch item, query): slices are visited in ascending order and
// hold ascending index ranges, so strict `<` keeps the lowest index among equal d2.
template <bool WITH_INDEX>
__global__ __launch_bounds__(256) void nn_merge_kernel(const float* __restrict__ part_d2, const int* __restrict__ part_idx,
                                                       long part_stride, int slices, long total, float* __restrict__ dist_out,
                                                       int* __restrict__ idx_out) {
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    float best = INFINITY;
    int besti = -1;
    for (int s = 0; s < slices; ++s) {
        const float d = part_d2[(long)s * part_stride + o];
        if (WITH_INDEX) {
            if (d < best) { best = d; besti = part_idx[(long)s * part_stride + o]; }
        } else {
            best = fminf(best, d);
        }
    }
    if (dist_out) dist_out[o] = __fsqrt_rn(best);
    if (WITH_INDEX) idx_out[o] = besti;
}

int nn_slices(int n_query, int n_ref, int batch, int ref_slices) {
    const int max_slices = min(NN_MAX_SLICES, max(1, n_ref));
    if (ref_slices > 0) return min(ref_slices, max_slices);
    const long items = (long)batch * ceil_div(n_query, NN_TILE);
    const long want = (2L * m324::cu_count() + items - 1) / items;        // two work items per CU before slicing stops
    const long room = max(1, n_ref / NN_MIN_SLICE);
    return (int)max(1L, min(min(want, room), (long)max_slices));
}

// ---- fixed-order block sum of one double per thread (256 threads); every thread gets the total ----
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

constexpr int STAT_BLOCKS = 32;      // per-workgroup partials of one batch item (m324_dist_stats)

__global__ __launch_bounds__(256) void dist_stats_partial_kernel(const float* __restrict__ dist, int n, double threshold,
                                                                 double* __restrict__ partial) {
    __shared__ double sh[256];
    const int b = blockIdx.y;
    const float* d = dist + (long)b * n;
    double sum = 0.0, cnt = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += STAT_BLOCKS * 256) {
        const double v = (double)d[i];
        sum += v;
        cnt += v < threshold ? 1.0 : 0.0;
    }
    sum = block_sum_256(sum, sh);
    cnt = block_sum_256(cnt, sh);
    if (threadIdx.x == 0) {
        partial[((long)b * STAT_BLOCKS + blockIdx.x) * 2] = sum;
        partial[((long)b * STAT_BLOCKS + blockIdx.x) * 2 + 1] = cnt;
    }
}

__global__ __launch_bounds__(64) void dist_stats_finish_kernel(const double* __restrict__ partial, int batch, double* __restrict__ sum,
                                                               long long* __restrict__ count) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    double s = 0.0, c = 0.0;
    for (int i = 0; i < STAT_BLOCKS; ++i) {
        s += partial[((long)b * STAT_BLOCKS + i) * 2];
        c += partial[((long)b * STAT_BLOCKS + i) * 2 + 1];
    }
    sum[b] = s;
    count[b] = (long long)c;
}

// out = s * (R x) + t in fp64, rounded once to fp32.  params = {s, R[0][0..2], R[1][0..2], R[2][0..2], t[0..2]} (13 doubles).
__device__ __forceinline__ void transform_point(const double* __restrict__ prm, double x, double y, double z, double (&o)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = prm[0] * (x * prm[1 + 3 * i] + y * prm[2 + 3 * i] + z * prm[3 + 3 * i]) + prm[10 + i];
}

__global__ __launch_bounds__(256) void transform_points_kernel(const float* __restrict__ x, long n, const double* __restrict__ params,
                                                               float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double o[3];
    transform_point(params, (double)x[i * 3], (double)x[i * 3 + 1], (double)x[i * 3 + 2], o);
    out[i * 3] = (float)o[0];
    out[i * 3 + 1] = (float)o[1];
    out[i * 3 + 2] = (float)o[2];
}

constexpr int MOM_BLOCKS = 64;       // per-workgroup partials of m324_icp_moments
constexpr int MOM_REC = 32;          // doubles per record (30 used)

// record: [0] n, [1] sum |st - m|, [2..4] sum st, [5..7] sum m, [8..16] sum st (x) m (row = st component),
//         [17..19] sum x, [20..28] sum x (x) m, [29] sum |x|^2, [30..31] zero
__global__ __launch_bounds__(256) void icp_moments_partial_kernel(const float* __restrict__ src, int n, const double* __restrict__ params,
                                                                  const float* __restrict__ target, int n_target,
                                                                  const int* __restrict__ index, double* __restrict__ partial) {
    __shared__ double sh[256];
    double acc[30];
#pragma unroll
    for (int k = 0; k < 30; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += MOM_BLOCKS * 256) {
        const double x[3] = {(double)src[(long)i * 3], (double)src[(long)i * 3 + 1], (double)src[(long)i * 3 + 2]};
        double st[3], m[3];
        transform_point(params, x[0], x[1], x[2], st);
        const int j = index[i];
        const bool ok = j >= 0 && j < n_target;               // an unmatched point poisons the sums instead of reading out of bounds
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = ok ? (double)target[(long)j * 3 + c] : (double)NAN;
        const double dx = st[0] - m[0], dy = st[1] - m[1], dz = st[2] - m[2];
        acc[0] += 1.0;
        acc[1] += sqrt(dx * dx + dy * dy + dz * dz);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[2 + c] += st[c];
            acc[5 + c] += m[c];
            acc[17 + c] += x[c];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                acc[8 + 3 * c + e] += st[c] * m[e];
                acc[20 + 3 * c + e] += x[c] * m[e];
            }
        }
        acc[29] += x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    }
#pragma unroll
    for (int k = 0; k < 30; ++k) {
        const double v = block_sum_256(acc[k], sh);
        if (threadIdx.x == 0) partial[(long)blockIdx.x * MOM_REC + k] = v;
    }
}

__global__ __launch_bounds__(64) void icp_moments_finish_kernel(const double* __restrict__ partial, double* __restrict__ record) {
    const int k = threadIdx.x;
    if (k >= MOM_REC) return;
    double s = 0.0;
    if (k < 30)
        for (int b = 0; b < MOM_BLOCKS; ++b) s += partial[(long)b * MOM_REC + k];
    record[k] = s;
}

}  // namespace

extern "C" int m324_nn_plan(int n_query, int n_ref, int batch, int ref_slices, long* scratch_bytes) {
    M324_REQUIRE(n_query > 0 && n_ref > 0 && batch > 0 && ref_slices >= 0, "m324_nn_plan: sizes must be positive (n_query=%d n_ref=%d batch=%d ref_slices=%d)",
                 n_query, n_ref, batch, ref_slices);
    M324_REQUIRE((long)batch * ceil_div(n_query, NN_TILE) * NN_MAX_SLICES < 2147483647L, "m324_nn_plan: batch * query tiles too large");
    const int slices = nn_slices(n_query, n_ref, batch, ref_slices);
    if (scratch_bytes) *scratch_bytes = (long)slices * batch * n_query * 8;
    return slices;
}

extern "C" int m324_nn_search(const float* query, long stride_q, int n_query, const float* ref, long stride_r, int n_ref, int batch,
                              float* dist, int* index, int ref_slices, void* scratch, long scratch_bytes, void* stream) {
    M324_REQUIRE(query && ref, "m324_nn_search: null query or reference");
    M324_REQUIRE(dist || index, "m324_nn_search: both outputs are null");
    M324_REQUIRE(n_query > 0 && n_ref > 0 && batch > 0 && ref_slices >= 0 && stride_q >= 0 && stride_r >= 0,
                 "m324_nn_search: sizes must be positive (n_query=%d n_ref=%d batch=%d ref_slices=%d)", n_query, n_ref, batch, ref_slices);
    long need = 0;
    const int slices = m324_nn_plan(n_query, n_ref, batch, ref_slices, &need);
    if (slices < 0) return slices;
    M324_REQUIRE(slices == 1 || (scratch && scratch_bytes >= need), "m324_nn_search: %d reference slices need %ld scratch bytes, got %ld",
                 slices, need, scratch ? scratch_bytes : 0L);
    const int qtiles = ceil_div(n_query, NN_TILE);
    const int per_slice = ceil_div(n_ref, slices);
    const long total = (long)batch * n_query;
    float* part_d2 = (float*)scratch;
    int* part_idx = (int*)(part_d2 + (long)slices * total);
    const dim3 grid(batch * qtiles * slices), block(NN_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define NN_LAUNCH(WI, FIN)                                                                                                        \
    hipLaunchKernelGGL((nn_search_kernel<WI, FIN>), grid, block, 0, st, query, stride_q, n_query, ref, stride_r, n_ref, qtiles,   \
                       slices, per_slice, dist, index, part_d2, part_idx, total)
    if (slices == 1) {
        if (index) NN_LAUNCH(true, true); else NN_LAUNCH(false, true);
    } else {
        if (index) NN_LAUNCH(true, false); else NN_LAUNCH(false, false);
        const dim3 mgrid(ceil_div(total, 256));
        if (index)
            hipLaunchKernelGGL(nn_merge_kernel<true>, mgrid, dim3(256), 0, st, part_d2, part_idx, total, slices, total, dist, index);
        else
            hipLaunchKernelGGL(nn_merge_kernel<false>, mgrid, dim3(256), 0, st, part_d2, part_idx, total, slices, total, dist, index);
    }
#undef NN_LAUNCH
    M324_CHECK_LAUNCH("m324_nn_search");
    return M324_OK;
}

extern "C" int m324_dist_stats(const float* dist, int n, int batch, double threshold, double* partial, double* sum, long long* count,
                               void* stream) {
    M324_REQUIRE(dist && partial && sum && count && n > 0 && batch > 0 && batch <= 65535, "m324_dist_stats: bad arguments");
    hipLaunchKernelGGL(dist_stats_partial_kernel, dim3(STAT_BLOCKS, batch), dim3(256), 0, (hipStream_t)stream, dist, n, threshold, partial);
    hipLaunchKernelGGL(dist_stats_finish_kernel, dim3(ceil_div(batch, 64)), dim3(64), 0, (hipStream_t)stream, partial, batch, sum, count);
    M324_CHECK_LAUNCH("m324_dist_stats");
    return M324_OK;
}

extern "C" int m324_transform_points(const float* x, long n, const double* params, float* out, void* stream) {
    M324_REQUIRE(x && params && out && n > 0 && n < (1L << 31), "m324_transform_points: bad arguments");
    hipLaunchKernelGGL(transform_points_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n, params, out);
    M324_CHECK_LAUNCH("m324_transform_points");
    return M324_OK;
}

extern "C" int m324_icp_moments(const float* src, int n, const double* params, const float* target, int n_target, const int* index,
                                double* partial, double* record, void* stream) {
    M324_REQUIRE(src && params && target && index && partial && record && n > 0 && n_target > 0, "m324_icp_moments: bad arguments");
    hipLaunchKernelGGL(icp_moments_partial_kernel, dim3(MOM_BLOCKS), dim3(256), 0, (hipStream_t)stream, src, n, params, target, n_target,
                       index, partial);
    hipLaunchKernelGGL(icp_moments_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, record);
    M324_CHECK_LAUNCH("m324_icp_moments");
    return M324_OK;
}
