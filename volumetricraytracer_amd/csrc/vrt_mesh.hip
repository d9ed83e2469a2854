/* vrt_mesh.hip — vrt_volume_extract_mesh (include/vrt.h), kernels to driver: the zero surface of (field - iso) over a box of a resident
 * volume as an indexed triangle mesh, by naive surface nets.  The rule is csrc/mesh_core.h; the walk over runs of 64 cells, the runs'
 * records, their scan and the corner loads are csrc/grid_device.h's.
 *
 * Run order followed by lane order IS the order of the cells' keys, and the quads of a sample go with the cell whose corner 0 it is —
 * the same order.
 *   count   one record per run (16 B): the 64-bit mask of its active cells from __ballot, its vertex count and its quad count; the
 *           active cells' bounding box goes into partial records by atomic min / max, which no order of waves can change.
 *   scan    launch_run_scan: the counts become the runs' first vertex and first quad; the host reads the totals.
 *   emit    a run with a non-empty mask writes its vertices at first + popcount(mask below the lane) and its quads likewise; a
 *           neighbour cell's vertex number is one 16-byte load of its run's record and a popcount.  No N^3 index volume, no atomics:
 *           the output does not depend on how the device schedules its waves. */
#include <hip/hip_runtime.h>

#include <math.h>

#include "mesh_core.h"
#include "grid_device.h"
#include "vrt_context.h"

namespace vrt {

namespace {

template <bool TEXEL16>
__global__ __launch_bounds__(256) void mesh_count_kernel(const float* __restrict__ dense, RunGrid G, float iso, Run* __restrict__ runs,
                                                         unsigned n_runs, DBrushSlot* __restrict__ slots) {
    const unsigned r = blockIdx.x * kRunsPerBlock + (threadIdx.x >> 6);
    if (r >= n_runs) return; /* the whole wave */
    const int lane = (int)(threadIdx.x & 63u);
    int c[3];
    unsigned classes = 0u;
    if (cell_of(G, r, lane, c)) {
        float f[8];
        load_corners(dense, G.N, c, iso, TEXEL16, f);
        classes = vrt_mesh::corner_classes(f);
    }
    const bool act = vrt_mesh::active(classes);
    const unsigned quads = act ? vrt_mesh::owned_quads(classes, c, G.lo) : 0u;
    const u64 mask = __ballot(act);
    const unsigned n_quads = (unsigned)(__popcll(__ballot(quads & 1u)) + __popcll(__ballot(quads & 2u)) + __popcll(__ballot(quads & 4u)));
    if (lane != 0) return;
    Run rec;
    rec.mask = mask, rec.count[0] = (unsigned)__popcll(mask), rec.count[1] = n_quads; /* vertices and quads */
    runs[r] = rec;
    if (mask != 0ull) {
        EditReport report;
        bound_run(report, G.N, c, mask);
        report.write(slots, r);
    }
}

/* The vertex number of the active cell c of the cell box. */
__device__ __forceinline__ uint32_t vertex_number(const RunGrid& G, const Run* __restrict__ runs, const int c[3]) {
    const int rx = c[0] - G.lo[0], ry = c[1] - G.lo[1], rz = c[2] - G.lo[2];
    const Run rec = runs[((size_t)rx * G.n[2] + rz) * G.runs_y + (ry >> 6)];
    return number_in(rec, ry & 63);
}

template <bool TEXEL16>
__global__ __launch_bounds__(256) void mesh_emit_kernel(const float* __restrict__ dense, const uint8_t* __restrict__ material, RunGrid G, float iso,
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
        load_corners(dense, G.N, c, iso, TEXEL16, f);
        classes = vrt_mesh::corner_classes(f);
        const unsigned at = number_in(rec, lane);
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
    unsigned at = rec.count[1] + (unsigned)(__popcll(bx & below) + __popcll(by & below) + __popcll(bz & below));
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

/* the cells of the samples lo..hi, inclusive: a row of s samples has s - 1 cells */
RunGrid mesh_grid(int N, const int lo_xyz[3], const int hi_xyz[3]) {
    const int last[3] = {hi_xyz[0] - 1, hi_xyz[1] - 1, hi_xyz[2] - 1};
    return run_grid(N, lo_xyz, last);
}

/* scratch: mesh_scratch_bytes(grid) of device memory — the totals, the scan's block sums and one 16-byte record per run —, valid from
   launch_mesh_count to launch_mesh_emit. */
size_t mesh_scratch_bytes(const RunGrid& G) { return run_scratch_bytes(runs_of(G)); }

/* device memory: vertices (low half) and quads (high half) of the whole mesh after launch_mesh_count */
const unsigned long long* mesh_totals(const void* scratch) { return static_cast<const unsigned long long*>(scratch); }

/* Counts every run's vertices and quads and turns the counts into the runs' first vertex and first quad (a prefix sum in run order);
   slots: zeroed, then the active cells' box in inv_lo / hi1 (the edit report, vrt_launch.h; `counts` stays 0).  Not for an
   empty grid. */
hipError_t launch_mesh_count(const float* dense, bool texel16, const RunGrid& G, float iso, void* scratch, DBrushSlot* slots, hipStream_t stream) {
    if (no_cells(G)) return hipErrorInvalidValue;
    hipError_t e = clear_report(slots, stream);
    if (e != hipSuccess) return e;
    const unsigned n_runs = runs_of(G);
    Run* runs = records_of(scratch, n_runs);
    const dim3 grid((n_runs + kRunsPerBlock - 1) / kRunsPerBlock);
    if (texel16)
        hipLaunchKernelGGL(mesh_count_kernel<true>, grid, dim3(256), 0, stream, dense, G, iso, runs, n_runs, slots);
    else
        hipLaunchKernelGGL(mesh_count_kernel<false>, grid, dim3(256), 0, stream, dense, G, iso, runs, n_runs, slots);
    launch_run_scan(runs, n_runs, scratch, stream);
    return hipGetLastError();
}

/* Writes the vertices (3 floats of object space, 3 floats of normal, 1 material byte each) and the quads (6 indices each) at their
   numbers; any output may be NULL and is skipped.  vertex_cap / quad_cap: what the outputs hold. */
hipError_t launch_mesh_emit(const float* dense, const uint8_t* material, bool texel16, const RunGrid& G, float iso, float cell, float extent,
                            void* scratch, float* positions, float* normals, uint8_t* materials, uint32_t* indices, unsigned vertex_cap,
                            unsigned quad_cap, hipStream_t stream) {
    if (no_cells(G)) return hipErrorInvalidValue;
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
    const RunGrid grid = mesh_grid(N, lo, hi);
    DeviceState& D = ctx->dev[0];
    if (!no_cells(grid)) {
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
