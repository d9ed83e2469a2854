/* vrt_redistance.hip — vrt_volume_redistance (include/vrt.h), kernels to driver: the samples of a box of a resident volume rewritten as the
 * signed distance, within a band, to the zero surface of the field the slot holds.  The rule is csrc/redistance_core.h.
 *
 * Two passes over 8^3-sample tiles aligned with the grid.  The surfel pass (one wave per tile of the box grown by band + 1) classifies
 * the samples, turns the interface samples into surfels (centre and normal, 24 B) and keeps them compact: a first run counts and
 * reserves each tile's range with one atomic add, the host sizes the buffer from the total, a second run writes.  The distance pass
 * (one workgroup per tile of the box) walks the ranges of the tiles one or two rings around its own, staged in LDS as
 * structure-of-arrays and read at wave-uniform addresses, and keeps the smallest squared distance of each of its samples.  It writes
 * the dense grid in place: it reads nothing of the grid but its own samples, and the surfels were finished on the stream before. */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "redistance_core.h"
#include "edit_report.h"
#include "vrt_context.h"

namespace vrt {

namespace {

using vrt_redist::kTile;

constexpr size_t kHeaderBytes = 256; /* the surfel counter, ahead of the tile table */
constexpr int kChunk = 256;          /* surfels staged per round of the distance pass: one per lane */
constexpr int kMaxRing = 2;
constexpr int kMaxTiles = (2 * kMaxRing + 1) * (2 * kMaxRing + 1) * (2 * kMaxRing + 1);

struct TileRange {
    unsigned start, count;
};

__device__ __forceinline__ float decoded(const float* __restrict__ dense, size_t i, bool texel16) {
    const float s = dense[i];
    return vrt_redist::clamped(vrt_grid::decode(s, texel16));
}

/* One wave per tile; lane = (z, y) of the tile, looping over x.  A sample of the grown box g (grid order {x, z, y}, inclusive) that has
 * a 6-neighbour of the other class and is of a class `from` admits makes a surfel.  EMIT = false: counts, reserves the tile's range
 * (table[tile] = {start, count}; *counter grows to the total).  EMIT = true: writes the surfels into the reserved range, below cap. */
template <bool EMIT>
__global__ __launch_bounds__(64) void redist_surfel_kernel(const float* __restrict__ dense, int texel16, int N, int from, EditBox g, int t_lo_x,
                                                           int t_lo_z, int t_lo_y, unsigned* __restrict__ counter,
                                                           TileRange* __restrict__ table, float* __restrict__ surfels, unsigned cap) {
    const int T = (N + kTile - 1) / kTile;
    const int ty = t_lo_y + (int)blockIdx.x, tz = t_lo_z + (int)blockIdx.y, tx = t_lo_x + (int)blockIdx.z;
    const size_t tile = ((size_t)tx * T + tz) * T + ty;
    const int l = (int)threadIdx.x;
    const int y = ty * kTile + (l & 7), z = tz * kTile + (l >> 3);
    const bool row_in = z >= g.lo[1] && z < g.lo[1] + g.n[1] && y >= g.lo[2] && y < g.lo[2] + g.n[2];
    unsigned base = 0u, mine = 0u;
    if (EMIT) {
        const TileRange r = table[tile];
        if (r.count == 0u) return;
        base = r.start;
    }
    for (int k = 0; k < kTile; k++) {
        const int x = tx * kTile + k;
        bool is_surfel = false;
        vrt_redist::Surfel s;
        if (row_in && x >= g.lo[0] && x < g.lo[0] + g.n[0]) { /* the grown box is clipped to the grid */
            const size_t i = vrt_grid::index(N, x, y, z);
            const float e = decoded(dense, i, texel16);
            const bool out = vrt_redist::outside(e);
            /* xyz order: x, y, z */
            const bool hp[3] = {x + 1 < N, y + 1 < N, z + 1 < N}, hm[3] = {x > 0, y > 0, z > 0};
            const size_t step[3] = {(size_t)N * N, 1, (size_t)N};
            float ep[3], em[3];
            bool other = false;
            for (int a = 0; a < 3; a++) {
                ep[a] = hp[a] ? decoded(dense, i + step[a], texel16) : e;
                em[a] = hm[a] ? decoded(dense, i - step[a], texel16) : e;
                other = other || vrt_redist::outside(ep[a]) != out || vrt_redist::outside(em[a]) != out;
            }
            is_surfel = other && (from == VRT_REDISTANCE_FROM_BOTH || (from == VRT_REDISTANCE_FROM_OUTSIDE) == out);
            if (EMIT && is_surfel) {
                const int q[3] = {x, y, z};
                s = vrt_redist::surfel_of(q, e, ep, em, hp, hm);
            }
        }
        if (EMIT) {
            const unsigned long long vote = __ballot(is_surfel);
            if (is_surfel) {
                const unsigned at = base + (unsigned)__popcll(vote & ((1ull << l) - 1ull));
                if (at < cap) {
                    float* o = surfels + (size_t)at * 6;
                    o[0] = s.c[0], o[1] = s.c[1], o[2] = s.c[2], o[3] = s.n[0], o[4] = s.n[1], o[5] = s.n[2];
                }
            }
            base += (unsigned)__popcll(vote);
        } else {
            mine += is_surfel ? 1u : 0u;
        }
    }
    if (!EMIT) {
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
        if (l == 0 && mine != 0u) {
            TileRange r;
            r.start = atomicAdd(counter, mine);
            r.count = mine;
            table[tile] = r;
        }
    }
}

/* One workgroup of 256 lanes per tile of the box b (grid order, inclusive of lo, n samples); a lane owns the samples (x, z, y) and
 * (x + 4, z, y) of the tile.  Every surfel of the tiles `ring` rings around is met by every sample: the culled minimum of the contract. */
template <bool TEXEL16>
__global__ __launch_bounds__(256) void redist_distance_kernel(float* __restrict__ dense, int N, int band, int ring, float unit, EditBox b,
                                                              int t_lo_x, int t_lo_z, int t_lo_y, const TileRange* __restrict__ table,
                                                              const float* __restrict__ surfels, DBrushSlot* __restrict__ slots) {
    __shared__ unsigned t_start[kMaxTiles], t_first[kMaxTiles + 1]; /* a tile's range, and where it begins in the run of all of them */
    __shared__ float sc[6][kChunk];
    const int T = (N + kTile - 1) / kTile;
    const int ty = t_lo_y + (int)blockIdx.x, tz = t_lo_z + (int)blockIdx.y, tx = t_lo_x + (int)blockIdx.z;
    const int tid = (int)threadIdx.x;
    const int side = 2 * ring + 1, n_tiles = side * side * side;
    if (tid < n_tiles) {
        const int nx = tx + tid / (side * side) - ring, nz = tz + (tid / side) % side - ring, ny = ty + tid % side - ring;
        TileRange r = {0u, 0u};
        if (nx >= 0 && nx < T && nz >= 0 && nz < T && ny >= 0 && ny < T) r = table[((size_t)nx * T + nz) * T + ny];
        t_start[tid] = r.start;
        t_first[tid + 1] = r.count;
    }
    __syncthreads();
    if (tid == 0) { /* counts -> running sums */
        unsigned sum = 0u;
        t_first[0] = 0u;
        for (int t = 0; t < n_tiles; t++) {
            sum += t_first[t + 1];
            t_first[t + 1] = sum;
        }
    }
    __syncthreads();
    const unsigned total = t_first[n_tiles];

    const int y = ty * kTile + (tid & 7), z = tz * kTile + ((tid >> 3) & 7), x0 = tx * kTile + (tid >> 6), x1 = x0 + 4;
    const bool row_in = z >= b.lo[1] && z < b.lo[1] + b.n[1] && y >= b.lo[2] && y < b.lo[2] + b.n[2];
    const bool in0 = row_in && x0 >= b.lo[0] && x0 < b.lo[0] + b.n[0], in1 = row_in && x1 >= b.lo[0] && x1 < b.lo[0] + b.n[0];
    const size_t i0 = vrt_grid::index(N, x0, y, z), i1 = vrt_grid::index(N, x1, y, z);
    bool out0 = false, out1 = false; /* the class, read before anything is stored */
    if (in0) out0 = vrt_redist::outside(vrt_redist::clamped(vrt_grid::decode(dense[i0], TEXEL16)));
    if (in1) out1 = vrt_redist::outside(vrt_redist::clamped(vrt_grid::decode(dense[i1], TEXEL16)));
    const float px0 = (float)x0, px1 = (float)x1, py = (float)y, pz = (float)z;
    float best0 = INFINITY, best1 = INFINITY;

    for (unsigned off = 0u; off < total; off += (unsigned)kChunk) {
        const unsigned n = min(total - off, (unsigned)kChunk);
        if ((unsigned)tid < n) {
            const unsigned v = off + (unsigned)tid; /* the v-th surfel of the run: in the last tile that begins at or before v */
            int lo = 0, hi = n_tiles - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (t_first[mid] <= v) lo = mid; else hi = mid - 1;
            }
            const float* s = surfels + ((size_t)t_start[lo] + (v - t_first[lo])) * 6;
#pragma unroll
            for (int c = 0; c < 6; c++) sc[c][tid] = s[c];
        }
        __syncthreads();
        for (unsigned j = 0u; j < n; j++) {
            const float cx = sc[0][j], cy = sc[1][j], cz = sc[2][j], nx = sc[3][j], ny = sc[4][j], nz = sc[5][j];
            best0 = fminf(best0, vrt_redist::disc_d2(px0, py, pz, cx, cy, cz, nx, ny, nz));
            best1 = fminf(best1, vrt_redist::disc_d2(px1, py, pz, cx, cy, cz, nx, ny, nz));
        }
        __syncthreads();
    }

    EditReport report;
    const auto store = [&](size_t i, int x, float best, bool is_out) {
        const float D = vrt_redist::banded(best, band);
        const float m = vrt_redist::signed_value(D, unit, is_out);
        dense[i] = TEXEL16 ? vrt_grid::texel16_value(m) : m;
        report.add(N, x, y, z, D < (float)band); /* high half: the near samples */
    };
    if (in0) store(i0, x0, best0, out0);
    if (in1) store(i1, x1, best1, out1);
    const unsigned block = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    report.commit(slots, block * 4u + (unsigned)(tid >> 6));
}

int tiles_of(int N) { return (N + kTile - 1) / kTile; }
unsigned* counter_of(void* table) { return static_cast<unsigned*>(table); }
TileRange* ranges_of(void* table) { return reinterpret_cast<TileRange*>(static_cast<char*>(table) + kHeaderBytes); }

/* The tiles a sample box meets: first tile and tile count per grid axis. */
void tile_span(const EditBox& box, int first[3], dim3& grid) {
    unsigned n[3];
    for (int a = 0; a < 3; a++) {
        first[a] = box.lo[a] / kTile;
        n[a] = (unsigned)((box.lo[a] + box.n[a] - 1) / kTile - first[a] + 1);
    }
    grid = dim3(n[2], n[1], n[0]); /* y fastest, like the grid */
}

/* table: redistance_table_bytes(N) of device memory — the surfel counter and one
   {start, count} range per 8^3 tile of the grid —, valid from launch_redistance_count to launch_redistance_distance.  grown: the box
   grown by band + 1 and clipped to the grid; boxes are in the grid's own axis order like every EditBox. */
size_t redistance_table_bytes(int N) {
    const size_t T = (size_t)tiles_of(N);
    return kHeaderBytes + T * T * T * sizeof(TileRange);
}

size_t redistance_surfel_bytes(unsigned surfels) { return std::max<size_t>(surfels, 1) * 6 * sizeof(float); }

/* device memory: the total after launch_redistance_count */
const unsigned* redistance_surfel_count(const void* table) { return static_cast<const unsigned*>(table); }

/* Zeroes the table, then counts the surfels of every tile of `grown` and reserves their ranges. */
hipError_t launch_redistance_count(const float* dense, bool texel16, int N, int from, const EditBox& grown, void* table, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(table, 0, redistance_table_bytes(N), stream);
    if (e != hipSuccess) return e;
    int first[3];
    dim3 grid;
    tile_span(grown, first, grid);
    hipLaunchKernelGGL(redist_surfel_kernel<false>, grid, dim3(64), 0, stream, dense, (int)texel16, N, from, grown, first[0], first[1], first[2],
                       counter_of(table), ranges_of(table), static_cast<float*>(nullptr), 0u);
    return hipGetLastError();
}

/* Writes the surfels (centre xyz, normal xyz: 24 B) into their tiles' ranges; `capacity` surfels fit. */
hipError_t launch_redistance_surfels(const float* dense, bool texel16, int N, int from, const EditBox& grown, void* table, void* surfels,
                                     unsigned capacity, hipStream_t stream) {
    int first[3];
    dim3 grid;
    tile_span(grown, first, grid);
    hipLaunchKernelGGL(redist_surfel_kernel<true>, grid, dim3(64), 0, stream, dense, (int)texel16, N, from, grown, first[0], first[1], first[2],
                       counter_of(table), ranges_of(table), static_cast<float*>(surfels), capacity);
    return hipGetLastError();
}

/* Every sample of `box` stores its banded signed distance (its texel when texel16), in place; slots: zeroed, then the written samples'
   box and count (the edit report, vrt_launch.h), with the count of samples nearer than the band in the high half of `counts`. */
hipError_t launch_redistance_distance(bool texel16, float* dense, int N, int band, float unit, const EditBox& box, const void* table,
                                      const void* surfels, DBrushSlot* slots, hipStream_t stream) {
    if (band < 1 || band > vrt_redist::kMaxBand) return hipErrorInvalidValue;
    hipError_t e = clear_report(slots, stream);
    if (e != hipSuccess) return e;
    int first[3];
    dim3 grid;
    tile_span(box, first, grid);
    const int ring = vrt_redist::tile_rings(band);
    const TileRange* ranges = ranges_of(const_cast<void*>(table));
    if (texel16)
        hipLaunchKernelGGL(redist_distance_kernel<true>, grid, dim3(256), 0, stream, dense, N, band, ring, unit, box, first[0], first[1], first[2],
                           ranges, static_cast<const float*>(surfels), slots);
    else
        hipLaunchKernelGGL(redist_distance_kernel<false>, grid, dim3(256), 0, stream, dense, N, band, ring, unit, box, first[0], first[1], first[2],
                           ranges, static_cast<const float*>(surfels), slots);
    return hipGetLastError();
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_redistance_result) == 48, "vrt.h states this size");

extern "C" {

/* vrt_volume_redistance: first, on every device, the surfels of the box grown by band + 1 are counted (launch_redistance_count) and the
 * buffer that holds them is grown — nothing of the volume has been written when that fails —; then per device the surfels are written,
 * the box's samples become banded signed distances in place (launch_redistance_distance, which reports like a brush launch), and what
 * the slot derives from the samples is recomputed over the box (rebuild_derived).  Afterwards every buffer equals what upload_volume
 * builds from the redistanced volume. */
int vrt_volume_redistance(vrt_ctx* ctx, int slot, int band, int from, const int* origin, const int* size, vrt_redistance_result* result) {
    if (!ctx) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    if (band < 1 || band > vrt_redist::kMaxBand) return VRT_ERR_INVALID;
    if (from != VRT_REDISTANCE_FROM_BOTH && from != VRT_REDISTANCE_FROM_OUTSIDE && from != VRT_REDISTANCE_FROM_INSIDE) return VRT_ERR_INVALID;
    HostVolume& h = ctx->vol[slot];
    const int N = h.N;
    int lo[3], hi[3], glo[3], ghi[3];
    int rc = clip_box(N, origin, size, lo, hi);
    if (rc != VRT_OK) return rc;
    for (int a = 0; a < 3; a++) {
        glo[a] = std::max(lo[a] - vrt_redist::cull_reach(band), 0);
        ghi[a] = std::min(hi[a] + vrt_redist::cull_reach(band), N - 1);
    }
    const EditBox box = derived_boxes(h, lo, hi).samples;
    const EditBox grown = derived_boxes(h, glo, ghi).samples;
    const bool texel16 = h.format == VRT_FORMAT_TEXEL16;
    const float cell = (h.extent * 2.0f) / (float)(N - 1);
    const float unit = cell / h.density_scale;
    std::vector<unsigned> surfels(ctx->dev.size(), 0u);
    Edit e;
    e.slot = slot;
    e.foot = box;
    e.rebuild = Edit::kFootprint; /* the requested box, whatever was reported */
    e.prepare = [&](DeviceState& D, size_t di) -> int {
        int rc = ensure_buffer(D.buf[kBufRedistTable], redistance_table_bytes(N));
        if (rc != VRT_OK) return rc;
        HIP_TRY(launch_redistance_count(D.vol[slot].dense, texel16, N, from, grown, D.buf[kBufRedistTable].p, D.stream));
        HIP_TRY(hipMemcpyAsync(&surfels[di], redistance_surfel_count(D.buf[kBufRedistTable].p), sizeof(unsigned), hipMemcpyDeviceToHost, D.stream));
        HIP_TRY(hipStreamSynchronize(D.stream));
        return ensure_buffer(D.buf[kBufRedistSurfels], redistance_surfel_bytes(surfels[di]));
    };
    e.write = [&](DeviceState& D, size_t di) -> int {
        DeviceVolume& v = D.vol[slot];
        if (surfels[di] > 0u)
            HIP_TRY(launch_redistance_surfels(v.dense, texel16, N, from, grown, D.buf[kBufRedistTable].p, D.buf[kBufRedistSurfels].p, surfels[di], D.stream));
        HIP_TRY(launch_redistance_distance(texel16, v.dense, N, band, unit, box, D.buf[kBufRedistTable].p, D.buf[kBufRedistSurfels].p, D.d_brush, D.stream));
        return VRT_OK;
    };
    e.reported = [&](const Written& got) {
        if (result)
            *result = vrt_redistance_result{{got.lo[0], got.lo[1], got.lo[2]}, {got.hi[0], got.hi[1], got.hi[2]}, got.low, got.high, surfels[0], 0};
    };
    return run_edit(ctx, e);
}

}  // extern "C"
