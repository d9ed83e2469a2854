/* vrt_fill.hip — vrt_volume_fill_enclosed (include/vrt.h), kernels to driver: which passable samples (d > 0) of a resident volume the
 * grid's faces cannot reach through 6-neighbour steps over passable samples, and the edit that turns them solid.
 *
 * Labels ("exterior") live in a scratch buffer next to the passable mask, both as bits: a row of samples along y is row_bytes(N)
 * bytes, sample y at bit y & 7 of byte y >> 3 — an 8^3 tile owns one byte of each of its 64 rows.  Labels only ever go from 0 to 1 and
 * a byte is written by its tile alone, so a tile that reads a neighbour's byte while that neighbour runs sees an older or a newer
 * state of a set that only grows towards the same fixed point: every order of the workgroups gives the same labels.  There is no wait
 * on another workgroup anywhere: convergence comes from the host launching rounds until one changes nothing. */
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>

#include "fill_core.h"
#include "edit_report.h"
#include "vrt_context.h"

namespace vrt {

namespace {

using vrt_fill::kTile;

constexpr size_t kFlagBytes = 256; /* the rounds' flags, ahead of the two bit grids */
constexpr int kFillRoundsPerRead = 8; /* propagation rounds enqueued between two reads of their flags: one stream sync per batch */
static_assert(kFillRoundsPerRead * sizeof(int) <= kFlagBytes, "one flag per round of a batch");

/* Passable mask of every row byte, and the seeds: the passable samples with an index 0 or N - 1 on some axis.  One lane per byte:
 * 8 consecutive samples along y. */
__global__ __launch_bounds__(256) void fill_mask_kernel(const float* __restrict__ dense, int texel16, int N, uint8_t* __restrict__ pas,
                                                        uint8_t* __restrict__ lab) {
    const int T = vrt_fill::row_bytes(N);
    const size_t count = (size_t)N * N * T;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) {
        const size_t row = i / (size_t)T; /* x * N + z */
        const int t = (int)(i % (size_t)T);
        const int x = (int)(row / (size_t)N), z = (int)(row % (size_t)N);
        unsigned p = 0u;
        for (int k = 0; k < kTile; k++) {
            const int y = t * kTile + k;
            if (y >= N) break;
            const float s = dense[row * N + y];
            p |= vrt_fill::passable(vrt_grid::decode(s, texel16)) ? 1u << k : 0u;
        }
        unsigned face = 0xffu;
        if (x > 0 && x < N - 1 && z > 0 && z < N - 1) face = (t == 0 ? 1u : 0u) | (t == (N - 1) / kTile ? 1u << ((N - 1) % kTile) : 0u);
        pas[i] = (uint8_t)p;
        lab[i] = (uint8_t)(p & face);
    }
}

/* One round: one workgroup (one wave) per 8^3 tile.  The tile's 64 rows and the rows one sample around them come into LDS as 10-bit
 * columns — bit 0 the sample below the tile, bits 1..8 the tile's, bit 9 the one above —, lane lx * 8 + lz owns row (lx, lz); the tile
 * then propagates labels over its own passable samples until nothing changes, writes the rows that changed and raises the round's flag.
 * A tile without an unlabelled passable sample leaves at once. */
constexpr int kHalo = kTile + 2;
__global__ __launch_bounds__(64) void fill_round_kernel(int N, const uint8_t* __restrict__ pas, uint8_t* lab, int* __restrict__ flag) {
    const int T = vrt_fill::row_bytes(N);
    const int ty = (int)blockIdx.x, tz = (int)blockIdx.y, tx = (int)blockIdx.z;
    const int l = (int)threadIdx.x, lx = l >> 3, lz = l & 7;
    const int x = tx * kTile + lx, z = tz * kTile + lz;
    const bool inside = x < N && z < N;
    const size_t mine_at = ((size_t)x * N + z) * T + ty;
    const unsigned passm = inside ? (unsigned)pas[mine_at] << 1 : 0u;
    const unsigned loaded = inside ? (unsigned)lab[mine_at] << 1 : 0u;
    if (!__any((passm & ~loaded) != 0u)) return;

    __shared__ unsigned col[kHalo * kHalo];
    for (int c = l; c < kHalo * kHalo; c += 64) {
        const int cx = tx * kTile + c / kHalo - 1, cz = tz * kTile + c % kHalo - 1;
        unsigned w = 0u;
        if (cx >= 0 && cx < N && cz >= 0 && cz < N) {
            const uint8_t* row = lab + ((size_t)cx * N + cz) * T;
            w = (unsigned)row[ty] << 1;
            if (ty > 0) w |= (unsigned)row[ty - 1] >> 7;
            if (ty + 1 < T) w |= ((unsigned)row[ty + 1] & 1u) << 9;
        }
        col[c] = w;
    }
    __syncthreads();
    const int own = (lx + 1) * kHalo + (lz + 1);
    unsigned mine = col[own];
    bool tile_changed = false;
    for (int it = 0; it <= kTile * kTile * kTile; it++) { /* every pass but the last labels a sample: at most 8^3 of them */
        const unsigned around = col[own - kHalo] | col[own + kHalo] | col[own - 1] | col[own + 1];
        unsigned cur = mine | (around & passm);
#pragma unroll
        for (int k = 0; k < kTile; k++) cur |= ((cur << 1) | (cur >> 1)) & passm; /* along y, from the tile's and the halo's bits */
        const bool changed = cur != mine;
        if (!__any(changed)) break;
        __syncthreads(); /* every lane has read this pass's columns */
        if (changed) col[own] = mine = cur;
        tile_changed = true;
        __syncthreads();
    }
    if (!tile_changed) return;
    if (((mine ^ loaded) & 0x1feu) != 0u) lab[mine_at] = (uint8_t)(mine >> 1); /* never outside the grid: passm is 0 there */
    if (l == 0) *flag = 1;
}

/* One lane per sample, y fastest like the dense grid: an enclosed sample (passable, not labelled) stores m = -(d + wall) — its texel in
 * a TEXEL16 slot — and, with material_id >= 0, that id.  Counts and box go into an EditReport (edit_report.h). */
template <bool TEXEL16>
__global__ __launch_bounds__(256) void fill_apply_kernel(float* __restrict__ dense, uint8_t* __restrict__ material, int N,
                                                         const uint8_t* __restrict__ pas, const uint8_t* __restrict__ lab, float wall,
                                                         int material_id, DBrushSlot* __restrict__ slots) {
    const int T = vrt_fill::row_bytes(N);
    const size_t count = (size_t)N * N * N;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    EditReport report;
    for (; i < count; i += stride) {
        const size_t row = i / (size_t)N;
        const int y = (int)(i % (size_t)N);
        const size_t at = row * T + (size_t)(y / kTile);
        if ((((unsigned)pas[at] & ~(unsigned)lab[at]) >> (y % kTile) & 1u) == 0u) continue;
        const int x = (int)(row / (size_t)N), z = (int)(row % (size_t)N);
        const float stored = dense[i];
        const float m = vrt_fill::filled_density(vrt_grid::decode(stored, TEXEL16), wall);
        dense[i] = TEXEL16 ? vrt_grid::texel16_value(m) : m;
        if (material_id >= 0) material[i] = (uint8_t)material_id;
        report.add(N, x, y, z, true); /* every write is a density write */
    }
    report.commit(slots, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
}

size_t bits_bytes(int N) { return (size_t)N * N * vrt_fill::row_bytes(N); }
uint8_t* pas_of(void* scratch) { return static_cast<uint8_t*>(scratch) + kFlagBytes; }
uint8_t* lab_of(void* scratch, int N) { return pas_of(scratch) + bits_bytes(N); }
unsigned stride_grid(size_t count) { return (unsigned)std::max<size_t>(1, std::min<size_t>((count + 255) / 256, 1u << 16)); }

/* scratch: fill_scratch_bytes(N) of device memory holding the flags of a batch of rounds, the
   passable mask and the exterior labels (one bit per sample each), valid from launch_fill_mask to launch_fill_apply. */
size_t fill_scratch_bytes(int N) { return kFlagBytes + 2 * bits_bytes(N); }

/* the flags of a batch of rounds (device memory) */
const int* fill_round_flags(const void* scratch) { return static_cast<const int*>(scratch); }

/* The mask of the samples with d > 0 (a TEXEL16 field decoded) and the seeds: those of them on a face of the grid. */
hipError_t launch_fill_mask(const float* dense, bool texel16, int N, void* scratch, hipStream_t stream) {
    hipLaunchKernelGGL(fill_mask_kernel, dim3(stride_grid(bits_bytes(N))), dim3(256), 0, stream, dense, (int)texel16, N, pas_of(scratch),
                       lab_of(scratch, N));
    return hipGetLastError();
}

/* `rounds` (1 .. kFillRoundsPerRead) propagation rounds, one workgroup per 8^3 tile each; round r sets fill_round_flags(scratch)[r]
   (device memory, zeroed first) when it labelled a sample.  A round that labelled none has reached the exterior set. */
hipError_t launch_fill_rounds(int N, void* scratch, int rounds, hipStream_t stream) {
    if (rounds < 1 || rounds > kFillRoundsPerRead) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(scratch, 0, kFlagBytes, stream);
    if (e != hipSuccess) return e;
    const unsigned T = (unsigned)vrt_fill::row_bytes(N);
    for (int r = 0; r < rounds; r++)
        hipLaunchKernelGGL(fill_round_kernel, dim3(T, T, T), dim3(64), 0, stream, N, pas_of(scratch), lab_of(scratch, N),
                           static_cast<int*>(scratch) + r);
    return hipGetLastError();
}

/* Every passable sample without a label stores -(d + wall) (its texel when texel16) and, material_id >= 0, that id; slots: zeroed, then
   the written samples' counts and box (the edit report, vrt_launch.h). */
hipError_t launch_fill_apply(bool texel16, float* dense, uint8_t* material, int N, const void* scratch, float wall, int material_id,
                             DBrushSlot* slots, hipStream_t stream) {
    hipError_t e = clear_report(slots, stream);
    if (e != hipSuccess) return e;
    void* s = const_cast<void*>(scratch);
    const unsigned grid = stride_grid((size_t)N * N * N);
    if (texel16)
        hipLaunchKernelGGL(fill_apply_kernel<true>, dim3(grid), dim3(256), 0, stream, dense, material, N, pas_of(s), lab_of(s, N), wall,
                           material_id, slots);
    else
        hipLaunchKernelGGL(fill_apply_kernel<false>, dim3(grid), dim3(256), 0, stream, dense, material, N, pas_of(s), lab_of(s, N), wall,
                           material_id, slots);
    return hipGetLastError();
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_fill_result) == 40, "vrt.h states this size");

extern "C" {

/* vrt_volume_fill_enclosed: per device, the passable mask and the face seeds (launch_fill_mask), propagation rounds in batches of
 * kFillRoundsPerRead with one read of their flags per batch until a round labels nothing, then the edit of the samples left without a
 * label (launch_fill_apply), which reports like a brush launch; what the slot derives from the samples is recomputed over the written
 * box (rebuild_derived).  The scratch memory of every device is there before the first sample is written.  Afterwards every buffer equals what upload_volume builds from the filled volume. */
int vrt_volume_fill_enclosed(vrt_ctx* ctx, int slot, float wall, int material, vrt_fill_result* result) {
    if (!ctx) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    if (!std::isfinite(wall) || wall < 0.f || material < -1 || material > 255) return VRT_ERR_INVALID;
    HostVolume& h = ctx->vol[slot];
    const int N = h.N;
    if (result) *result = vrt_fill_result{{N, N, N}, {-1, -1, -1}, 0, 0, 0};
    const bool texel16 = h.format == VRT_FORMAT_TEXEL16;
    /* a round that changes something labels at least one sample, so no run needs more rounds than the grid has samples */
    const unsigned long long round_cap = (unsigned long long)N * N * N + 1ull;
    const int zero[3] = {0, 0, 0}, last[3] = {N - 1, N - 1, N - 1};
    unsigned long long rounds = 0; /* of the device whose `write` ran last: device 0's when `reported` reads it */
    Edit e;
    e.slot = slot;
    e.foot = derived_boxes(h, zero, last).samples;
    e.rebuild = Edit::kWrites; /* every written sample is a density write */
    e.prepare = [&](DeviceState& D, size_t) { return ensure_buffer(D.buf[kBufFill], fill_scratch_bytes(N)); };
    /* mask and rounds write the scratch only; the volume's first write is launch_fill_apply */
    e.write = [&](DeviceState& D, size_t) -> int {
        DeviceVolume& v = D.vol[slot];
        HIP_TRY(launch_fill_mask(v.dense, texel16, N, D.buf[kBufFill].p, D.stream));
        rounds = 0;
        for (bool settled = false; !settled;) {
            if (rounds >= round_cap) {
                fprintf(stderr, "[vrt] vrt_volume_fill_enclosed: %llu rounds without settling on a grid of %d^3\n", rounds, N);
                return VRT_ERR_HIP;
            }
            int flags[kFillRoundsPerRead];
            HIP_TRY(launch_fill_rounds(N, D.buf[kBufFill].p, kFillRoundsPerRead, D.stream));
            HIP_TRY(hipMemcpyAsync(flags, fill_round_flags(D.buf[kBufFill].p), sizeof flags, hipMemcpyDeviceToHost, D.stream));
            HIP_TRY(hipStreamSynchronize(D.stream));
            rounds += kFillRoundsPerRead;
            for (int f : flags) settled = settled || f == 0;
        }
        HIP_TRY(launch_fill_apply(texel16, v.dense, v.material, N, D.buf[kBufFill].p, wall, material, D.d_brush, D.stream));
        return VRT_OK;
    };
    e.reported = [&](const Written& got) {
        if (result)
            *result = vrt_fill_result{{got.lo[0], got.lo[1], got.lo[2]}, {got.hi[0], got.hi[1], got.hi[2]}, got.low,
                                      (uint32_t)std::min<unsigned long long>(rounds, 0xffffffffull), 0};
    };
    return run_edit(ctx, e);
}

}  // extern "C"
