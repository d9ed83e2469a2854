/* vrt_measure.hip — vrt_volume_measure and vrt_measure_properties (include/vrt.h), kernels to driver: how much of a resident volume
 * there is and where it sits, as integer sums over a box of its samples.  The rule is csrc/measure_core.h.
 *
 * One pass, one kernel.  The unit of work is a run (csrc/grid_device.h, as in vrt_mesh.hip): 64 consecutive samples along y of one
 * (x, z) row of the SAMPLE box, one wave, lane = sample = the cell whose corner 0 it is.  A workgroup (4 waves) walks over runs with
 * the grid's stride, so the number of atomics does not grow with the box.
 *   loads   a lane reads its cell's eight corners straight from the grid, each guarded by the box: a sample is read by the (at most)
 *           eight cells around it, a bounded number of times, and the rows of a run are whole 256-byte lines that the caches serve
 *           to the neighbouring rows.  This is what the mesh count pass does, at 66 us for 257^3; an LDS tile with its apron would
 *           save cache hits, not memory traffic, and would tie the run to a tile shape that boxes with odd origins do not have.
 *           A wave walks over some eighty runs of a 257^3 grid at four waves per SIMD, so it is the latency of these loads that it
 *           would wait for: the loads of the wave's next run (nine per lane, the material id among them) are issued before the
 *           current run is summed.
 *   counts  solid samples are a ballot and a popcount, wave-uniform in a scalar register; crossings, active cells and quads are
 *           counted by the lane that sees them and added across the lanes at the end.
 *   cells   a cell whose corners are all INSIDE adds its closed form in its own lane.  The active cells of a run — almost none, or a
 *           handful — are compacted by the ballot's mask: for each set bit the wave reads that lane's eight corner values with
 *           v_readlane and its 64 lanes evaluate the cell's 64 sub-samples, one each; no lane idles while another works through 64.
 *   area    the lane that owns a quad recomputes the vertices of its three other cells (24 loads per quad, cache hits next to the
 *           surface) and keeps the quantised area in a 64-bit integer of its own.
 *   sums    every value is an integer: per lane in registers across the runs, then across the wave by __shfl_xor, then across the
 *           workgroup in LDS (with a 256-bin histogram of material ids, which a wave feeds with one add when its solid samples share
 *           an id), then one 64-bit vector atomic per non-zero value and workgroup.  The cells' box goes the same way with integer min
 *           and max.  No floating-point atomics: the result does not depend on how the device schedules its waves.
 * Designed for 4 waves per SIMD (at most 128 VGPRs), no scratch memory, no spills: tests/test_measure_kernel_resources.py. */
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>

#include "measure_core.h"
#include "grid_device.h"
#include "vrt_context.h"

namespace vrt {

namespace {

/* The accumulators, 64-bit words: what vrt_measure_result sums, the material counts, and (two 32-bit halves to a word) the cells' box. */
enum { kS0 = 0, kS1 = 1, kS2 = 4, kSolid = 10, kActive = 11, kCross = 12, kQuads = 15, kArea = 16, kSumWords = 17, kMaterial = 17,
       kBox = kMaterial + 256, kWords = kBox + 3 };
constexpr int kWavesPerBlock = 4;
constexpr unsigned kMaxBlocks = 1024; /* 256 CUs x 4 SIMDs x 4 waves */

__global__ __launch_bounds__(320) void measure_clear_kernel(u64* __restrict__ acc, int N) {
    const unsigned i = threadIdx.x;
    if (i < (unsigned)kBox) acc[i] = 0ull;
    if (i < 6u) reinterpret_cast<int*>(acc + kBox)[i] = i < 3u ? N : -1;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float lane_value(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

/* Lane `lane` of run r: where its sample sits in the box, whether it lies in the box (live) and whether its neighbour one index up
   on each axis does (more). */
struct BoxLane : RunPlace {
    bool live, more[3];
    __device__ __forceinline__ BoxLane(const RunGrid& G, unsigned r, int lane) : RunPlace(run_place(G, r, lane)) {
        live = rel_y < G.n[1];
        more[0] = rx + 1 < G.n[0], more[1] = rel_y + 1 < G.n[1], more[2] = rz + 1 < G.n[2];
    }
    /* corner j of the lane's cell is a sample of the box */
    __device__ __forceinline__ bool in_box(int j) const { return live && (!(j & 1) || more[0]) && (!(j & 2) || more[1]) && (!(j & 4) || more[2]); }
};

/* What a lane reads of its run: the stored floats of its cell's corners (0 for a corner beyond the box, which is not read) and its
   sample's material id. */
struct Fetched {
    float stored[8];
    int id;
};
__device__ __forceinline__ Fetched fetch(const float* __restrict__ dense, const uint8_t* __restrict__ material, const RunGrid& G, unsigned r,
                                         int lane) {
    const BoxLane at(G, r, lane);
    const size_t i0 = vrt_grid::index(G.N, G.lo[0] + at.rx, G.lo[1] + at.rel_y, G.lo[2] + at.rz);
    Fetched out;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const size_t i = i0 + (size_t)(j & 1) * G.N * G.N + (size_t)((j >> 1) & 1) + (size_t)(j >> 2) * G.N;
        out.stored[j] = at.in_box(j) ? dense[i] : 0.0f;
    }
    out.id = at.live ? (int)material[i0] : 0;
    return out;
}

template <bool TEXEL16>
__global__ __launch_bounds__(256) void measure_kernel(const float* __restrict__ dense, const uint8_t* __restrict__ material, RunGrid G, float iso,
                                                      unsigned n_runs, u64* __restrict__ acc) {
    namespace M = vrt_mesh;
    namespace R = vrt_measure;
    __shared__ u64 part[kSumWords];
    __shared__ unsigned hist[256];
    __shared__ int box[6];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6); /* the same in every lane: a run's row arithmetic stays in scalar registers */
    hist[tid] = 0u;
    if (tid < kSumWords) part[tid] = 0ull;
    if (tid < 6) box[tid] = tid < 3 ? INT_MAX : -1;
    __syncthreads();

    R::Sums sums;
    R::clear(sums);
    u64 area = 0ull;
    int blo[3] = {INT_MAX, INT_MAX, INT_MAX}, bhi[3] = {-1, -1, -1};
    unsigned n_solid = 0u;                               /* wave-uniform, from the ballot the histogram needs anyway */
    unsigned n_active = 0u, n_quads = 0u, n_cross[3] = {0u, 0u, 0u}; /* the lane's own; a lane sees at most 3 * 513^3 / 64 */
    const int ix = lane & 3, iy = (lane >> 2) & 3, iz = lane >> 4;                          /* the lane's sub-sample of a shared cell */

    const unsigned stride = gridDim.x * kWavesPerBlock;
    Fetched next = {};
    unsigned r =blockIdx.x * kWavesPerBlock + (unsigned)w;
    if (r < n_runs) next = fetch(dense, material, G, r, lane);
    for (; r < n_runs; r += stride) {
        const Fetched now = next;
        if (r + stride < n_runs) next = fetch(dense, material, G, r + stride, lane); /* in flight while this run is summed */
        const BoxLane at(G, r, lane);
        const int rx = at.rx, rz = at.rz, rel_y = at.rel_y;
        const unsigned ry = at.ry;
        const int c[3] = {G.lo[0] + rx, G.lo[1] + rel_y, G.lo[2] + rz};
        const bool live = at.live;
        const bool more[3] = {at.more[0], at.more[1], at.more[2]};
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; j++) f[j] = at.in_box(j) ? M::field(vrt_grid::decode(now.stored[j], TEXEL16), iso) : -0.0f;
        /* the sample: its class, its material id, the three edges that start at it */
        const bool solid = live && !M::outside(f[0]);
        const u64 solid_mask = __ballot(solid);
        n_solid += (unsigned)__popcll(solid_mask);
#pragma unroll
        for (int a = 0; a < 3; a++) n_cross[a] += live && more[a] && M::outside(f[0]) != M::outside(f[1 << a]) ? 1u : 0u;
        if (solid_mask != 0ull) {
            const int first_lane = (int)__ffsll((long long)solid_mask) - 1;
            const int id = solid ? now.id : -1;
            const int first = __builtin_amdgcn_readlane(id, first_lane);
            const u64 same = __ballot(id == first);
            if (lane == first_lane) atomicAdd(&hist[first], (unsigned)__popcll(same));
            if (solid && id != first) atomicAdd(&hist[id], 1u);
        }
        /* the cell */
        const bool is_cell = live && more[0] && more[1] && more[2];
        const unsigned classes = M::corner_classes(f);
        const bool act = is_cell && M::active(classes);
        const unsigned quads = act ? M::owned_quads(classes, c, G.lo) : 0u;
        u64 todo = __ballot(act);
        n_active += act ? 1u : 0u;
        n_quads += (unsigned)__popc(quads);
        bool counted = false; /* the cell has an INSIDE sub-sample */
        if (is_cell && classes == 0u) {
            R::add_full_cell(sums, c);
            counted = true;
        }
        while (todo != 0ull) { /* the wave's active cells, one after the other: lane = sub-sample */
            const int k = (int)__ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            float g[8];
#pragma unroll
            for (int j = 0; j < 8; j++) g[j] = lane_value(f[j], k);
            const bool inside = R::subsample_inside(g, ix, iy, iz);
            const u64 any = __ballot(inside);
            if (inside) {
                const uint32_t X[3] = {R::position(c[0], ix), R::position(G.lo[1] + (int)ry * 64 + k, iy), R::position(c[2], iz)};
                R::add_subsample(sums, X);
            }
            if (lane == k) counted = any != 0ull;
        }
        if (counted) {
#pragma unroll
            for (int a = 0; a < 3; a++) blo[a] = min(blo[a], c[a]), bhi[a] = max(bhi[a], c[a]);
        }
        /* the quads of the cell's corner 0: q2 is the cell itself */
        if (quads != 0u) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (!((quads >> a) & 1u)) continue;
                int cells[4][3];
                M::quad_cells(a, c, cells);
                float q[4][3];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    float g[8];
                    if (i == 2) {
#pragma unroll
                        for (int j = 0; j < 8; j++) g[j] = f[j];
                    } else {
                        load_corners(dense, G.N, cells[i], iso, TEXEL16, g);
                    }
                    const M::Vertex v = M::cell_vertex(cells[i], g);
                    q[i][0] = v.p[0], q[i][1] = v.p[1], q[i][2] = v.p[2];
                }
                area += R::quad_area_q(q, (classes & 1u) != 0u);
            }
        }
    }

    /* lanes -> wave -> workgroup -> one atomic per non-zero value */
    u64 mine[kSumWords];
    mine[kS0] = wave_sum(sums.s0);
#pragma unroll
    for (int a = 0; a < 3; a++) mine[kS1 + a] = wave_sum(sums.s1[a]);
#pragma unroll
    for (int a = 0; a < 6; a++) mine[kS2 + a] = wave_sum(sums.s2[a]);
    mine[kSolid] = n_solid, mine[kActive] = wave_sum((u64)n_active), mine[kQuads] = wave_sum((u64)n_quads);
#pragma unroll
    for (int a = 0; a < 3; a++) mine[kCross + a] = wave_sum((u64)n_cross[a]);
    mine[kArea] = wave_sum(area);
#pragma unroll
    for (int a = 0; a < 3; a++) blo[a] = wave_min(blo[a]), bhi[a] = wave_max(bhi[a]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kSumWords; i++)
            if (mine[i] != 0ull) atomicAdd(&part[i], mine[i]);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (bhi[a] >= 0) atomicMin(&box[a], blo[a]), atomicMax(&box[3 + a], bhi[a]);
        }
    }
    __syncthreads();
    if (tid < kSumWords && part[tid] != 0ull) atomicAdd(&acc[tid], part[tid]);
    if (hist[tid] != 0u) atomicAdd(&acc[kMaterial + tid], (u64)hist[tid]);
    int* out_box = reinterpret_cast<int*>(acc + kBox);
    if (tid < 3 && box[3 + tid] >= 0) atomicMin(&out_box[tid], box[tid]), atomicMax(&out_box[3 + tid], box[3 + tid]);
}

hipError_t launch_measure(const float* dense, const uint8_t* material, bool texel16, const RunGrid& G, float iso, u64* acc, hipStream_t stream) {
    const unsigned n_runs = runs_of(G);
    unsigned blocks = (n_runs + kWavesPerBlock - 1) / kWavesPerBlock;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    hipLaunchKernelGGL(measure_clear_kernel, dim3(1), dim3(320), 0, stream, acc, G.N);
    if (texel16)
        hipLaunchKernelGGL(measure_kernel<true>, dim3(blocks), dim3(256), 0, stream, dense, material, G, iso, n_runs, acc);
    else
        hipLaunchKernelGGL(measure_kernel<false>, dim3(blocks), dim3(256), 0, stream, dense, material, G, iso, n_runs, acc);
    return hipGetLastError();
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_measure_result) == 176, "vrt.h states this size");
static_assert(sizeof(vrt_mass_properties) == 136, "vrt.h states this size");
static_assert(kBox <= 320, "measure_clear_kernel clears one word per lane");

extern "C" {

/* vrt_volume_measure, on device 0: the accumulators are cleared, one launch sums over the runs of the sample box, and the host reads
 * the words back.  The slot is only read. */
int vrt_volume_measure(vrt_ctx* ctx, int slot, float iso, const int* origin, const int* size, vrt_measure_result* result, uint64_t* material_samples) {
    if (!ctx || !result || !std::isfinite(iso)) return VRT_ERR_INVALID;
    if ((origin == nullptr) != (size == nullptr)) return VRT_ERR_INVALID; /* ahead of the slot's check, as ever; clip_box needs the slot's N */
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    const HostVolume& h = ctx->vol[slot];
    const int N = h.N;
    int lo[3], hi[3];
    int rc = clip_box(N, origin, size, lo, hi);
    if (rc != VRT_OK) return rc;
    rc = quiesce(ctx);
    if (rc != VRT_OK) return rc;
    const RunGrid G = run_grid(N, lo, hi); /* the samples lo..hi */
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    rc = ensure_buffer(D.buf[kBufMeasure], kWords * sizeof(u64));
    if (rc != VRT_OK) return rc;
    u64* acc = static_cast<u64*>(D.buf[kBufMeasure].p);
    HIP_TRY(launch_measure(D.vol[slot].dense, D.vol[slot].material, h.format == VRT_FORMAT_TEXEL16, G, iso, acc, D.stream));
    u64 words[kWords];
    HIP_TRY(hipMemcpyAsync(words, acc, sizeof words, hipMemcpyDeviceToHost, D.stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    vrt_measure_result got = {};
    const int* cells = reinterpret_cast<const int*>(words + kBox);
    for (int a = 0; a < 3; a++) {
        got.lo[a] = cells[a], got.hi[a] = cells[3 + a];
        got.moment1[a] = words[kS1 + a], got.crossings[a] = words[kCross + a];
    }
    for (int a = 0; a < 6; a++) got.moment2[a] = words[kS2 + a];
    got.subsamples = words[kS0], got.solid_samples = words[kSolid], got.active_cells = words[kActive];
    got.quads = words[kQuads], got.area_q = words[kArea];
    *result = got;
    if (material_samples)
        for (int i = 0; i < 256; i++) material_samples[i] = words[kMaterial + i];
    return VRT_OK;
}

/* Host only: rule 7 of vrt_volume_measure, in double. */
int vrt_measure_properties(const vrt_measure_result* m, uint8_t resolution, float extent, vrt_mass_properties* out) {
    if (!m || !out || resolution > VRT_MAX_RESOLUTION) return VRT_ERR_INVALID;
    const int N = (1 << resolution) + 1;
    const double cell = (double)((extent * 2.0f) / (float)(N - 1)), h = cell / 8.0, e = (double)extent;
    vrt_mass_properties p = {};
    for (int a = 0; a < 3; a++) p.box_lo[a] = (double)m->lo[a] * cell - e, p.box_hi[a] = ((double)m->hi[a] + 1.0) * cell - e;
    if (m->subsamples != 0) { /* none: zeros, and lo > hi makes the box empty */
        /* a sub-sample stands for a cube of side s = cell / 4 = 2 h around it: s^3 of volume, s^5 / 12 of second moment of its own */
        const double S0 = (double)m->subsamples, s = 2.0 * h, s3 = s * s * s, h5 = (h * h) * s3, own = (s * s) * s3 / 12.0;
        const double S1[3] = {(double)m->moment1[0], (double)m->moment1[1], (double)m->moment1[2]};
        p.volume = S0 * s3;
        p.area = ((double)m->area_q / 65536.0) * (cell * cell);
        for (int a = 0; a < 3; a++) p.centroid[a] = (S1[a] / S0) * h - e;
        const int ia[6] = {0, 1, 2, 0, 0, 1}, ib[6] = {0, 1, 2, 1, 2, 2};
        double Cm[6];
        for (int i = 0; i < 6; i++) Cm[i] = ((double)m->moment2[i] - S1[ia[i]] * S1[ib[i]] / S0) * h5 + (i < 3 ? S0 * own : 0.0);
        const double tr = Cm[0] + Cm[1] + Cm[2];
        for (int i = 0; i < 6; i++) p.inertia[i] = (i < 3 ? tr : 0.0) - Cm[i];
    }
    *out = p;
    return VRT_OK;
}

}  // extern "C"
