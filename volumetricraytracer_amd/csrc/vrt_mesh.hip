/* vrt_mesh.hip — vrt_volume_extract_mesh (include/vrt.h), kernels to driver: the zero surface of (field - iso) over a box of a resident
 * volume as an indexed triangle mesh, by naive surface nets.  The rule is csrc/mesh_core.h.
 *
 * The unit of work is a run: 64 consecutive cells along y of one (x, z) row of the cell box, one wave, lane = cell.  Runs are numbered
 * in the grid's storage order (x slowest, then z, then y), so run order followed by lane order IS the order of the cells' keys, and
 * the quads of a sample go with the cell whose corner 0 it is — the same order.
 *   count   one record per run (16 B): the 64-bit mask of its active cells from __ballot, its vertex count and its quad count; the
 *           active cells' bounding box goes into partial records by atomic min / max, which no order of waves can change.
 *   scan    an exclusive prefix sum over the records' counts (three launches: block sums, their scan, the records), vertices and
 *           quads packed into one 64-bit word.  The counts become the runs' first vertex and first quad; the host reads the totals.
 *   emit    a run with a non-empty mask writes its vertices at first + popcount(mask below the lane) and its quads likewise; a
 *           neighbour cell's vertex number is one 16-byte load of its run's record and a popcount.  No N^3 index volume, no atomics:
 *           the output does not depend on how the device schedules its waves. */
#include <hip/hip_runtime.h>

#include <math.h>

#include "mesh_core.h"
#include "edit_report.h"
#include "vrt_context.h"

namespace vrt {

/* The cell box of a sample box, in xyz order (the mesh rule's own): its first cell, its cells
   per axis (one less than the samples; none when the box is one sample thick somewhere) and how many runs of 64 cells a row along y has. */
struct MeshGrid {
    int N;
    int lo[3];
    int n[3];
    int runs_y;
};

namespace {

constexpr int kRunsPerBlock = 4;  /* count / emit: 256 lanes, one run per wave */
constexpr int kScanThreads = 256; /* scan: each lane takes kScanItems consecutive records */
constexpr int kScanItems = 8;
constexpr size_t kHeaderBytes = 256; /* the packed totals, ahead of the block sums */

struct alignas(16) Run {
    unsigned long long mask; /* bit l: cell l of the run is active */
    unsigned v, q;           /* count: vertices and quads of the run; after the scan: its first vertex and first quad */
};

typedef unsigned long long u64;
__device__ __forceinline__ u64 packed(unsigned v, unsigned q) { return ((u64)q << 32) | (u64)v; }

/* The cell of lane `lane` of run r (xyz), and whether the row of the cell box reaches that far. */
__device__ __forceinline__ bool cell_of(const MeshGrid& G, unsigned r, int lane, int c[3]) {
    const unsigned ry = r % (unsigned)G.runs_y, t = r / (unsigned)G.runs_y;
    const int rel_y = (int)ry * 64 + lane;
    c[0] = G.lo[0] + (int)(t / (unsigned)G.n[2]);
    c[1] = G.lo[1] + rel_y;
    c[2] = G.lo[2] + (int)(t % (unsigned)G.n[2]);
    return rel_y < G.n[1];
}

/* The eight corner values of cell c; every corner of a cell of the cell box is a sample of the grid. */
template <bool TEXEL16>
__device__ __forceinline__ void load_corners(const float* __restrict__ dense, int N, const int c[3], float iso, float f[8]) {
    const size_t i0 = vrt_grid::index(N, c[0], c[1], c[2]);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const size_t i = i0 + (size_t)(j & 1) * N * N + (size_t)((j >> 1) & 1) + (size_t)(j >> 2) * N;
        const float s = dense[i];
        f[j] = vrt_mesh::field(vrt_grid::decode(s, TEXEL16), iso);
    }
}

template <bool TEXEL16>
__global__ __launch_bounds__(256) void mesh_count_kernel(const float* __restrict__ dense, MeshGrid G, float iso, Run* __restrict__ runs,
                                                         unsigned n_runs, DBrushSlot* __restrict__ slots) {
    const unsigned r = blockIdx.x * kRunsPerBlock + (threadIdx.x >> 6);
    if (r >= n_runs) return; /* the whole wave */
    const int lane = (int)(threadIdx.x & 63u);
    int c[3];
    unsigned classes = 0u;
    if (cell_of(G, r, lane, c)) {
        float f[8];
        load_corners<TEXEL16>(dense, G.N, c, iso, f);
        classes = vrt_mesh::corner_classes(f);
    }
    const bool act = vrt_mesh::active(classes);
    const unsigned quads = act ? vrt_mesh::owned_quads(classes, c, G.lo) : 0u;
    const u64 mask = __ballot(act);
    const unsigned n_quads = (unsigned)(__popcll(__ballot(quads & 1u)) + __popcll(__ballot(quads & 2u)) + __popcll(__ballot(quads & 4u)));
    if (lane != 0) return;
    Run rec;
    rec.mask = mask, rec.v = (unsigned)__popcll(mask), rec.q = n_quads;
    runs[r] = rec;
    if (mask != 0ull) { /* lane 0's cell is the run's first: x and z are the run's, y runs from the lowest to the highest set bit */
        const int y_lo = c[1] + (int)__ffsll((long long)mask) - 1, y_hi = c[1] + 63 - (int)__clzll((long long)mask);
        EditReport report; /* the ballot has folded the wave already: the run's two end cells say its box */
        report.bound(G.N, c[0], y_lo, c[2]);
        report.bound(G.N, c[0], y_hi, c[2]);
        report.write(slots, r);
    }
}

/* Exclusive prefix sum of v over the 256 lanes of the workgroup, and the sum of all of them; ends on a barrier, so that it can be
   called again. */
__device__ __forceinline__ u64 block_exclusive_scan(u64 v, u64& total, u64* wave_sum) {
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 below = __shfl_up(inc, o);
        if (lane >= o) inc += below;
    }
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    u64 before = 0ull, all = 0ull;
#pragma unroll
    for (int i = 0; i < kScanThreads / 64; i++) {
        const u64 s = wave_sum[i];
        before += i < w ? s : 0ull;
        all += s;
    }
    __syncthreads();
    total = all;
    return before + (inc - v);
}

/* sums[b]: the counts of the kScanThreads * kScanItems records of block b. */
__global__ __launch_bounds__(kScanThreads) void mesh_scan_reduce_kernel(const Run* __restrict__ runs, unsigned n_runs, u64* __restrict__ sums) {
    __shared__ u64 wave_sum[kScanThreads / 64];
    const size_t first = ((size_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
    u64 mine = 0ull;
#pragma unroll
    for (int j = 0; j < kScanItems; j++)
        if (first + j < n_runs) mine += packed(runs[first + j].v, runs[first + j].q);
    u64 total;
    (void)block_exclusive_scan(mine, total, wave_sum);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

/* One workgroup: sums -> their exclusive prefix sums, *totals = the sum of all. */
__global__ __launch_bounds__(kScanThreads) void mesh_scan_sums_kernel(u64* __restrict__ sums, unsigned n_blocks, u64* __restrict__ totals) {
    __shared__ u64 wave_sum[kScanThreads / 64];
    u64 carry = 0ull;
    for (unsigned base = 0u; base < n_blocks; base += kScanThreads) {
        const unsigned i = base + threadIdx.x;
        const u64 v = i < n_blocks ? sums[i] : 0ull;
        u64 total;
        const u64 ex = block_exclusive_scan(v, total, wave_sum);
        if (i < n_blocks) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *totals = carry;
}

/* The records' counts -> the runs' first vertex and first quad. */
__global__ __launch_bounds__(kScanThreads) void mesh_scan_apply_kernel(Run* __restrict__ runs, unsigned n_runs, const u64* __restrict__ sums) {
    __shared__ u64 wave_sum[kScanThreads / 64];
    const size_t first = ((size_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
    u64 count[kScanItems];
    u64 mine = 0ull;
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        count[j] = first + j < n_runs ? packed(runs[first + j].v, runs[first + j].q) : 0ull;
        mine += count[j];
    }
    u64 total;
    u64 at = sums[blockIdx.x] + block_exclusive_scan(mine, total, wave_sum);
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        if (first + j < n_runs) runs[first + j].v = (unsigned)at, runs[first + j].q = (unsigned)(at >> 32);
        at += count[j];
    }
}

/* The vertex number of the active cell c of the cell box. */
__device__ __forceinline__ uint32_t vertex_number(const MeshGrid& G, const Run* __restrict__ runs, const int c[3]) {
    const int rx = c[0] - G.lo[0], ry = c[1] - G.lo[1], rz = c[2] - G.lo[2];
    const Run rec = runs[((size_t)rx * G.n[2] + rz) * G.runs_y + (ry >> 6)];
    return rec.v + (uint32_t)__popcll(rec.mask & ((1ull << (ry & 63)) - 1ull));
}

template <bool TEXEL16>
__global__ __launch_bounds__(256) void mesh_emit_kernel(const float* __restrict__ dense, const uint8_t* __restrict__ material, MeshGrid G, float iso,
                                                        float cell, float extent, const Run* __restrict__ runs, unsigned n_runs,
                                                        float* __restrict__ positions, float* __restrict__ normals, uint8_t* __restrict__ materials,
                                                        uint32_t* __restrict__ indices, unsigned vertex_cap, unsigned quad_cap) {
    const unsigned r = blockIdx.x * kRunsPerBlock + (threadIdx.x >> 6);
    if (r >= n_runs) return; /* the whole wave */
    const Run rec = runs[r];
    if (rec.mask == 0ull) return; /* no vertex; and no quad, whose owner's cell is one of its four active cells */
    const int lane = (int)(threadIdx.x & 63u);
    const u64 below = (1ull << lane) - 1ull;
    int c[3];
    (void)cell_of(G, r, lane, c);
    const bool act = ((rec.mask >> lane) & 1ull) != 0ull;
    unsigned classes = 0u;
    if (act) {
        float f[8];
        load_corners<TEXEL16>(dense, G.N, c, iso, f);
        classes = vrt_mesh::corner_classes(f);
        const unsigned at = rec.v + (unsigned)__popcll(rec.mask & below);
        if (at < vertex_cap) {
            const vrt_mesh::Vertex v = vrt_mesh::cell_vertex(c, f);
            if (positions) {
                float* o = positions + (size_t)at * 3;
                o[0] = vrt_mesh::object_coordinate(v.p[0], cell, extent), o[1] = vrt_mesh::object_coordinate(v.p[1], cell, extent);
                o[2] = vrt_mesh::object_coordinate(v.p[2], cell, extent);
            }
            if (normals) {
                float* o = normals + (size_t)at * 3;
                o[0] = v.n[0], o[1] = v.n[1], o[2] = v.n[2];
            }
            if (materials) {
                const int j = vrt_mesh::material_corner(classes);
                const size_t i = ((size_t)(c[0] + (j & 1)) * G.N + (size_t)(c[2] + (j >> 2))) * G.N + (size_t)(c[1] + ((j >> 1) & 1));
                materials[at] = material[i];
            }
        }
    }
    const unsigned quads = act ? vrt_mesh::owned_quads(classes, c, G.lo) : 0u;
    const u64 bx = __ballot(quads & 1u), by = __ballot(quads & 2u), bz = __ballot(quads & 4u);
    if (!indices || quads == 0u) return;
    unsigned at = rec.q + (unsigned)(__popcll(bx & below) + __popcll(by & below) + __popcll(bz & below));
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (!((quads >> a) & 1u)) continue;
        int cells[4][3];
        vrt_mesh::quad_cells(a, c, cells);
        uint32_t q[4], out[6];
#pragma unroll
        for (int i = 0; i < 4; i++) q[i] = vertex_number(G, runs, cells[i]);
        vrt_mesh::quad_indices(q, (classes & 1u) != 0u, out);
        if (at < quad_cap) {
            uint32_t* o = indices + (size_t)at * 6;
#pragma unroll
            for (int i = 0; i < 6; i++) o[i] = out[i];
        }
        at++;
    }
}

unsigned runs_of(const MeshGrid& G) { return (unsigned)G.n[0] * (unsigned)G.n[2] * (unsigned)G.runs_y; }
unsigned scan_blocks_of(unsigned n_runs) { return (n_runs + kScanThreads * kScanItems - 1) / (kScanThreads * kScanItems); }
size_t sums_bytes(unsigned n_runs) { return ((size_t)scan_blocks_of(n_runs) * sizeof(u64) + 255) / 256 * 256; }
u64* totals_of(void* scratch) { return static_cast<u64*>(scratch); }
u64* sums_of(void* scratch) { return reinterpret_cast<u64*>(static_cast<char*>(scratch) + kHeaderBytes); }
Run* records_of(void* scratch, unsigned n_runs) { return reinterpret_cast<Run*>(static_cast<char*>(scratch) + kHeaderBytes + sums_bytes(n_runs)); }

/* the samples lo..hi, inclusive */
MeshGrid mesh_grid(int N, const int lo_xyz[3], const int hi_xyz[3]) {
    MeshGrid G;
    G.N = N;
    for (int a = 0; a < 3; a++) {
        G.lo[a] = lo_xyz[a];
        G.n[a] = hi_xyz[a] - lo_xyz[a]; /* a row of s samples has s - 1 cells */
    }
    G.runs_y = (G.n[1] + 63) / 64;
    return G;
}

bool mesh_grid_empty(const MeshGrid& G) { return G.n[0] < 1 || G.n[1] < 1 || G.n[2] < 1; }

/* scratch: mesh_scratch_bytes(grid) of device memory — the totals, the scan's block sums and one 16-byte record per run —, valid from
   launch_mesh_count to launch_mesh_emit. */
size_t mesh_scratch_bytes(const MeshGrid& G) {
    const unsigned n_runs = runs_of(G);
    return kHeaderBytes + sums_bytes(n_runs) + (size_t)n_runs * sizeof(Run);
}

/* device memory: vertices (low half) and quads (high half) of the whole mesh after launch_mesh_count */
const unsigned long long* mesh_totals(const void* scratch) { return static_cast<const unsigned long long*>(scratch); }

/* Counts every run's vertices and quads and turns the counts into the runs' first vertex and first quad (a prefix sum in run order);
   slots: zeroed, then the active cells' box in inv_lo / hi1 (the edit report, vrt_launch.h; `counts` stays 0).  Not for an
   empty grid. */
hipError_t launch_mesh_count(const float* dense, bool texel16, const MeshGrid& G, float iso, void* scratch, DBrushSlot* slots, hipStream_t stream) {
    if (mesh_grid_empty(G)) return hipErrorInvalidValue;
    hipError_t e = clear_report(slots, stream);
    if (e != hipSuccess) return e;
    const unsigned n_runs = runs_of(G), n_blocks = scan_blocks_of(n_runs);
    Run* runs = records_of(scratch, n_runs);
    const dim3 grid((n_runs + kRunsPerBlock - 1) / kRunsPerBlock);
    if (texel16)
        hipLaunchKernelGGL(mesh_count_kernel<true>, grid, dim3(256), 0, stream, dense, G, iso, runs, n_runs, slots);
    else
        hipLaunchKernelGGL(mesh_count_kernel<false>, grid, dim3(256), 0, stream, dense, G, iso, runs, n_runs, slots);
    hipLaunchKernelGGL(mesh_scan_reduce_kernel, dim3(n_blocks), dim3(kScanThreads), 0, stream, runs, n_runs, sums_of(scratch));
    hipLaunchKernelGGL(mesh_scan_sums_kernel, dim3(1), dim3(kScanThreads), 0, stream, sums_of(scratch), n_blocks, totals_of(scratch));
    hipLaunchKernelGGL(mesh_scan_apply_kernel, dim3(n_blocks), dim3(kScanThreads), 0, stream, runs, n_runs, sums_of(scratch));
    return hipGetLastError();
}

/* Writes the vertices (3 floats of object space, 3 floats of normal, 1 material byte each) and the quads (6 indices each) at their
   numbers; any output may be NULL and is skipped.  vertex_cap / quad_cap: what the outputs hold. */
hipError_t launch_mesh_emit(const float* dense, const uint8_t* material, bool texel16, const MeshGrid& G, float iso, float cell, float extent,
                            void* scratch, float* positions, float* normals, uint8_t* materials, uint32_t* indices, unsigned vertex_cap,
                            unsigned quad_cap, hipStream_t stream) {
    if (mesh_grid_empty(G)) return hipErrorInvalidValue;
    const unsigned n_runs = runs_of(G);
    const Run* runs = records_of(scratch, n_runs);
    const dim3 grid((n_runs + kRunsPerBlock - 1) / kRunsPerBlock);
    if (texel16)
        hipLaunchKernelGGL(mesh_emit_kernel<true>, grid, dim3(256), 0, stream, dense, material, G, iso, cell, extent, runs, n_runs, positions, normals,
                           materials, indices, vertex_cap, quad_cap);
    else
        hipLaunchKernelGGL(mesh_emit_kernel<false>, grid, dim3(256), 0, stream, dense, material, G, iso, cell, extent, runs, n_runs, positions, normals,
                           materials, indices, vertex_cap, quad_cap);
    return hipGetLastError();
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_mesh_result) == 40, "vrt.h states this size");

extern "C" {

/* vrt_volume_extract_mesh, on device 0: the runs of the cell box are counted and scanned (launch_mesh_count), the host reads the two
 * totals and the active cells' box, checks the caller's capacities and sizes the staged mesh, the runs write it (launch_mesh_emit) and
 * the arrays the caller asked for are copied out.  The slot is only read. */
int vrt_volume_extract_mesh(vrt_ctx* ctx, int slot, float iso, const int* origin, const int* size, float* positions, float* normals, uint8_t* materials,
                 size_t vertex_capacity, uint32_t* indices, size_t index_capacity, vrt_mesh_result* result) {
    if (!ctx || !std::isfinite(iso)) return VRT_ERR_INVALID;
    if ((origin == nullptr) != (size == nullptr)) return VRT_ERR_INVALID; /* ahead of the slot's check, as ever; clip_box needs the slot's N */
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    const HostVolume& h = ctx->vol[slot];
    const int N = h.N;
    int lo[3], hi[3];
    int rc = clip_box(N, origin, size, lo, hi);
    if (rc != VRT_OK) return rc;
    const bool wanted = positions || normals || materials || indices;
    const bool texel16 = h.format == VRT_FORMAT_TEXEL16;
    const float cell = (h.extent * 2.0f) / (float)(N - 1);
    rc = quiesce(ctx);
    if (rc != VRT_OK) return rc;
    vrt_mesh_result got = {{N, N, N}, {-1, -1, -1}, 0, 0};
    const MeshGrid grid = mesh_grid(N, lo, hi);
    DeviceState& D = ctx->dev[0];
    if (!mesh_grid_empty(grid)) {
        HIP_TRY(hipSetDevice(D.ordinal));
        rc = ensure_buffer(D.buf[kBufMeshScratch], mesh_scratch_bytes(grid));
        if (rc != VRT_OK) return rc;
        HIP_TRY(launch_mesh_count(D.vol[slot].dense, texel16, grid, iso, D.buf[kBufMeshScratch].p, D.d_brush, D.stream));
        unsigned long long totals = 0;
        Written cells; /* the active cells' box */
        HIP_TRY(hipMemcpyAsync(&totals, mesh_totals(D.buf[kBufMeshScratch].p), sizeof totals, hipMemcpyDeviceToHost, D.stream));
        rc = read_report(D, N, cells); /* the totals arrive in the same synchronisation */
        if (rc != VRT_OK) return rc;
        got = vrt_mesh_result{{cells.lo[0], cells.lo[1], cells.lo[2]}, {cells.hi[0], cells.hi[1], cells.hi[2]}, totals & 0xffffffffull, totals >> 32};
    }
    if (result) *result = got;
    if (!wanted) return VRT_OK;
    if (vertex_capacity < got.vertices || index_capacity < 6 * got.quads) return VRT_ERR_INVALID;
    if (got.vertices == 0) return VRT_OK;
    /* the staged mesh: positions, normals, indices, materials, each where the one before ends (all but the last a multiple of 4 bytes) */
    const size_t V = (size_t)got.vertices, Q = (size_t)got.quads;
    const size_t at_normals = V * 3 * sizeof(float), at_indices = at_normals * 2, at_materials = at_indices + Q * 6 * sizeof(uint32_t);
    rc = ensure_buffer(D.buf[kBufMeshOut], at_materials + V);
    if (rc != VRT_OK) return rc;
    char* out = static_cast<char*>(D.buf[kBufMeshOut].p);
    float* d_positions = positions ? reinterpret_cast<float*>(out) : nullptr;
    float* d_normals = normals ? reinterpret_cast<float*>(out + at_normals) : nullptr;
    uint32_t* d_indices = indices && Q ? reinterpret_cast<uint32_t*>(out + at_indices) : nullptr;
    uint8_t* d_materials = materials ? reinterpret_cast<uint8_t*>(out + at_materials) : nullptr;
    HIP_TRY(launch_mesh_emit(D.vol[slot].dense, D.vol[slot].material, texel16, grid, iso, cell, h.extent, D.buf[kBufMeshScratch].p, d_positions, d_normals,
                             d_materials, d_indices, (unsigned)V, (unsigned)Q, D.stream));
    if (d_positions) HIP_TRY(hipMemcpyAsync(positions, d_positions, at_normals, hipMemcpyDeviceToHost, D.stream));
    if (d_normals) HIP_TRY(hipMemcpyAsync(normals, d_normals, at_normals, hipMemcpyDeviceToHost, D.stream));
    if (d_indices) HIP_TRY(hipMemcpyAsync(indices, d_indices, Q * 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, D.stream));
    if (d_materials) HIP_TRY(hipMemcpyAsync(materials, d_materials, V, hipMemcpyDeviceToHost, D.stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    return VRT_OK;
}

}  // extern "C"
