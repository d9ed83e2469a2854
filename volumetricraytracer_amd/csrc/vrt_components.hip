/* vrt_components.hip — vrt_volume_components (include/vrt.h), kernels to driver: the 6-connected components of a resident volume's solid
 * samples (!(d > 0)), their sizes and boxes, and the edit that removes some of them.
 *
 * A label is one word per sample (components_core.h): a solid sample starts with its own key (x*N + z)*N + y, a passable one holds
 * kPassable.  Labels are parent links that only ever decrease, so every chain ends at a root (label == key), and a word read while
 * another workgroup lowers it gives some value it has held: an ancestor then and for ever.  Nothing waits on another workgroup.
 *   local    one wave per 8^3 tile: minimum propagation in LDS to the tile-local fixed point
 *   merge    every pair of face-adjacent solid samples in different tiles: a lock-free union of their roots (atomicMin of the lower
 *            root into the higher root's word)
 *   flatten  label = root, in a launch of its own: the kernel boundary makes the merge's words visible; counts the roots
 *   roots    every root takes a row of the component table and leaves its number in the second word grid
 *   stats    samples and box per component, by atomics into the table, folded in registers and across the wave first
 *   mark     the removal predicate (a mode and two scalars) sets kRemovedBit in the labels of the samples that go
 *   apply    one lane per sample: removed samples and their halo are written (rules 5 and 6), from the labels alone
 * Every find and every union loop is capped and raises a flag that the host turns into VRT_ERR_HIP. */
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <vector>

#include "components_core.h"
#include "fill_core.h" /* the 8^3 tiles and their row bytes */
#include "edit_report.h"
#include "vrt_context.h"

namespace vrt {

namespace {

using namespace vrt_components_core;
using vrt_fill::kTile;

/* the scratch memory: a header of counters, the labels, the second word grid (a root's row in the table) */
constexpr size_t kHeaderBytes = 256;
constexpr int kGaveUp = 0, kRoots = 1, kNextRow = 2; /* words of the header */
/* A chain visits roots of tile-local components with falling keys: it cannot be longer than the grid has samples, and it is far
   shorter; a union retries only when another lane has linked its root meanwhile. */
constexpr int kFindCap = 1 << 24, kUniteCap = 1 << 20;

__device__ __forceinline__ unsigned load_label(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

/* The root above label a.  Gives up (flag, and whatever it reached) after kFindCap steps. */
__device__ __forceinline__ unsigned find_root(const unsigned* lab, unsigned a, unsigned* header) {
    for (int s = 0; s < kFindCap; s++) {
        const unsigned p = load_label(lab + a);
        if (p == a) return a;
        a = p;
    }
    atomicOr(header + kGaveUp, 1u);
    return a;
}

/* The components of samples a and b become one. */
__device__ __forceinline__ void unite(unsigned* lab, unsigned a, unsigned b, unsigned* header) {
    for (int s = 0; s < kUniteCap; s++) {
        a = find_root(lab, a, header);
        b = find_root(lab, b, header);
        if (a == b) return;
        if (load_label(header + kGaveUp) != 0u) return;
        if (a > b) {
            const unsigned t = a;
            a = b, b = t;
        }
        const unsigned old = atomicMin(lab + b, a); /* b was a root: it now hangs below a */
        if (old == b) return;
        b = old; /* b had a parent already: that parent's tree and a's are the ones to join */
    }
    atomicOr(header + kGaveUp, 1u);
}

/* local: one workgroup (one wave) per 8^3 tile, lane lx * 8 + lz owns the row (lx, lz) of 8 samples along y and keeps their labels in
 * registers; LDS holds the tile's labels as [y][lane] for the four neighbouring rows to read.  A pass takes the minimum over the
 * solid 6-neighbours inside the tile — along y in registers, to the end of every run —; a pass that changes something lowers a label,
 * and a label has to travel at most 511 steps, so 512 passes always suffice.  A tile without a solid sample writes its kPassable words and
 * leaves. */
__global__ __launch_bounds__(64) void components_local_kernel(const float* __restrict__ dense, int texel16, int N, unsigned* __restrict__ lab) {
    const int ty = (int)blockIdx.x, tz = (int)blockIdx.y, tx = (int)blockIdx.z;
    const int l = (int)threadIdx.x, lx = l >> 3, lz = l & 7;
    const int x = tx * kTile + lx, z = tz * kTile + lz, y0 = ty * kTile;
    const bool inside = x < N && z < N;
    const unsigned base = inside ? key_of(N, x, y0, z) : 0u;
    unsigned mine[kTile];
    unsigned solid_mask = 0u;
#pragma unroll
    for (int k = 0; k < kTile; k++) {
        mine[k] = kPassable;
        if (inside && y0 + k < N) {
            const float s = dense[base + k];
            if (solid(vrt_grid::decode(s, texel16))) mine[k] = base + k, solid_mask |= 1u << k;
        }
    }
    if (__any(solid_mask != 0u)) {
        __shared__ unsigned tile[kTile * 64];
#pragma unroll
        for (int k = 0; k < kTile; k++) tile[k * 64 + l] = mine[k];
        __syncthreads();
        for (int pass = 0; pass < kTile * kTile * kTile; pass++) {
            unsigned next[kTile];
#pragma unroll
            for (int k = 0; k < kTile; k++) {
                unsigned m = mine[k];
                if (lx > 0) m = min(m, tile[k * 64 + l - 8]);
                if (lx < kTile - 1) m = min(m, tile[k * 64 + l + 8]);
                if (lz > 0) m = min(m, tile[k * 64 + l - 1]);
                if (lz < kTile - 1) m = min(m, tile[k * 64 + l + 1]);
                next[k] = (solid_mask >> k & 1u) ? m : kPassable;
            }
#pragma unroll
            for (int k = 1; k < kTile; k++)
                if (solid_mask >> k & 1u) next[k] = min(next[k], next[k - 1]);
#pragma unroll
            for (int k = kTile - 2; k >= 0; k--)
                if (solid_mask >> k & 1u) next[k] = min(next[k], next[k + 1]);
            bool changed = false;
#pragma unroll
            for (int k = 0; k < kTile; k++) changed = changed || next[k] != mine[k];
            if (!__any(changed)) break;
            __syncthreads(); /* every lane has read this pass's labels */
#pragma unroll
            for (int k = 0; k < kTile; k++) tile[k * 64 + l] = mine[k] = next[k];
            __syncthreads();
        }
    }
    if (!inside) return;
#pragma unroll
    for (int k = 0; k < kTile; k++)
        if (y0 + k < N) lab[base + k] = mine[k];
}

/* merge: one lane per sample, y fastest.  A solid sample whose neighbour one step up an axis lies in the next tile and is solid
 * unites with it; pairs are taken from their lower sample only. */
__global__ __launch_bounds__(256) void components_merge_kernel(int N, unsigned* lab, unsigned* header) {
    const size_t count = (size_t)N * N * N;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < count; i += stride) {
        const int y = (int)(i % (size_t)N);
        const size_t row = i / (size_t)N;
        const int x = (int)(row / (size_t)N), z = (int)(row % (size_t)N);
        const bool up_x = x % kTile == kTile - 1 && x + 1 < N, up_z = z % kTile == kTile - 1 && z + 1 < N;
        const bool up_y = y % kTile == kTile - 1 && y + 1 < N;
        if (!(up_x || up_y || up_z)) continue;
        if (!label_solid(load_label(lab + i))) continue;
        if (up_y && label_solid(load_label(lab + i + 1))) unite(lab, (unsigned)i, (unsigned)(i + 1), header);
        if (up_z && label_solid(load_label(lab + i + (size_t)N))) unite(lab, (unsigned)i, (unsigned)(i + (size_t)N), header);
        if (up_x && label_solid(load_label(lab + i + (size_t)N * N))) unite(lab, (unsigned)i, (unsigned)(i + (size_t)N * N), header);
    }
}

/* flatten: every solid sample's label becomes its root; a root never changes here, so a chain read while other lanes store still ends
 * at it.  The roots are counted, one atomic per wave. */
__global__ __launch_bounds__(256) void components_flatten_kernel(int N, unsigned* lab, unsigned* header) {
    const size_t count = (size_t)N * N * N;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    unsigned roots = 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const unsigned p = load_label(lab + i);
        if (!label_solid(p)) continue;
        if (p == (unsigned)i) {
            roots++;
            continue;
        }
        const unsigned r = find_root(lab, p, header);
        if (r != p) __hip_atomic_store(lab + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int o = 32; o > 0; o >>= 1) roots += __shfl_xor(roots, o);
    if ((threadIdx.x & 63u) == 0u && roots != 0u) atomicAdd(header + kRoots, roots);
}

/* One row of the component table (32 B): the box as an EditReport keeps it, growing from 0. */
struct DComponent {
    unsigned key, samples;
    unsigned inv_lo[3], hi1[3]; /* N - lowest, 1 + highest x, y, z */
};
static_assert(sizeof(DComponent) == 32, "components_table_bytes counts on it");

/* roots: every root takes the next row (one atomic per wave; the host orders the rows) and leaves its number at its own key. */
__global__ __launch_bounds__(256) void components_roots_kernel(int N, const unsigned* __restrict__ lab, unsigned* __restrict__ row_of,
                                                               DComponent* __restrict__ table, unsigned capacity, unsigned* header) {
    const size_t count = (size_t)N * N * N;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t rounds = (count + stride - 1) / stride; /* whole waves stay in the loop: the ballot below is the wave's */
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    for (size_t r = 0; r < rounds; r++, i += stride) {
        const bool root = i < count && lab[i] == (unsigned)i;
        const unsigned long long votes = __ballot(root);
        if (votes == 0ull) continue;
        unsigned first = 0u;
        if (lane == (unsigned)__ffsll((long long)votes) - 1u) first = atomicAdd(header + kNextRow, (unsigned)__popcll(votes));
        first = __shfl(first, __ffsll((long long)votes) - 1);
        if (!root) continue;
        const unsigned mine = first + (unsigned)__popcll(votes & ((1ull << lane) - 1ull));
        if (mine >= capacity) { /* more roots than flatten counted: never, and never out of bounds */
            atomicOr(header + kGaveUp, 1u);
            continue;
        }
        row_of[i] = mine;
        table[mine] = DComponent{(unsigned)i, 0u, {0u, 0u, 0u}, {0u, 0u, 0u}};
    }
}

/* stats: one lane per sample, y fastest, a bounded grid.  A lane sums the samples of one root in registers and goes to the table when
 * the root changes; at the end a wave whose lanes all hold the same root folds first and sends one set of atomics. */
struct Tally {
    unsigned root = kPassable, n = 0u;
    unsigned inv_lo_x = 0u, inv_lo_y = 0u, inv_lo_z = 0u, hi1_x = 0u, hi1_y = 0u, hi1_z = 0u;

    __device__ __forceinline__ void send(const unsigned* __restrict__ row_of, DComponent* __restrict__ table) const {
        if (n == 0u) return;
        DComponent* c = table + row_of[root];
        atomicAdd(&c->samples, n);
        atomicMax(&c->inv_lo[0], inv_lo_x), atomicMax(&c->inv_lo[1], inv_lo_y), atomicMax(&c->inv_lo[2], inv_lo_z);
        atomicMax(&c->hi1[0], hi1_x), atomicMax(&c->hi1[1], hi1_y), atomicMax(&c->hi1[2], hi1_z);
    }
};
__global__ __launch_bounds__(256) void components_stats_kernel(int N, const unsigned* __restrict__ lab, const unsigned* __restrict__ row_of,
                                                               DComponent* __restrict__ table) {
    const size_t count = (size_t)N * N * N;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    Tally t;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const unsigned r = lab[i];
        if (!label_solid(r)) continue;
        if (r != t.root) {
            t.send(row_of, table);
            t = Tally();
            t.root = r;
        }
        const int y = (int)(i % (size_t)N);
        const size_t row = i / (size_t)N;
        const int x = (int)(row / (size_t)N), z = (int)(row % (size_t)N);
        t.n++;
        t.inv_lo_x = max(t.inv_lo_x, (unsigned)(N - x)), t.inv_lo_y = max(t.inv_lo_y, (unsigned)(N - y)), t.inv_lo_z = max(t.inv_lo_z, (unsigned)(N - z));
        t.hi1_x = max(t.hi1_x, (unsigned)(x + 1)), t.hi1_y = max(t.hi1_y, (unsigned)(y + 1)), t.hi1_z = max(t.hi1_z, (unsigned)(z + 1));
    }
    /* lanes without a sample (root kPassable, n 0) go along with any root */
    unsigned common = t.n != 0u ? t.root : kPassable;
    for (int o = 32; o > 0; o >>= 1) common = min(common, __shfl_xor(common, o));
    if (__all(t.n == 0u || t.root == common)) {
        for (int o = 32; o > 0; o >>= 1) {
            t.n += __shfl_xor(t.n, o);
            t.inv_lo_x = max(t.inv_lo_x, __shfl_xor(t.inv_lo_x, o)), t.inv_lo_y = max(t.inv_lo_y, __shfl_xor(t.inv_lo_y, o));
            t.inv_lo_z = max(t.inv_lo_z, __shfl_xor(t.inv_lo_z, o));
            t.hi1_x = max(t.hi1_x, __shfl_xor(t.hi1_x, o)), t.hi1_y = max(t.hi1_y, __shfl_xor(t.hi1_y, o)), t.hi1_z = max(t.hi1_z, __shfl_xor(t.hi1_z, o));
        }
        t.root = common;
        if ((threadIdx.x & 63u) != 0u) return;
    }
    t.send(row_of, table);
}

/* mark: the samples of the components the predicate removes get kRemovedBit. */
__global__ __launch_bounds__(256) void components_mark_kernel(int N, unsigned* __restrict__ lab, const unsigned* __restrict__ row_of,
                                                              const DComponent* __restrict__ table, int mode, unsigned a, unsigned b) {
    const size_t count = (size_t)N * N * N;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const unsigned r = lab[i];
        if (!label_solid(r)) continue;
        const unsigned samples = mode == kRemoveBelow ? table[row_of[r]].samples : 0u;
        if (removed_by(mode, a, b, r, samples)) lab[i] = r | kRemovedBit;
    }
}

/* apply: one lane per sample, y fastest like the dense grid.  A sample of a removed component stores removed_density (its texel in a
 * TEXEL16 slot) and, with material_id >= 0, that id; a passable sample below the gap with a removed and without a kept 6-neighbour
 * stores the gap when that changes its bits.  Neighbours are read as labels only, never as densities: every decision is from the field
 * before the call.  Counts and box go into an EditReport (edit_report.h). */
template <bool TEXEL16>
__global__ __launch_bounds__(256) void components_apply_kernel(float* __restrict__ dense, uint8_t* __restrict__ material, int N,
                                                               const unsigned* __restrict__ lab, float gap, int material_id,
                                                               DBrushSlot* __restrict__ slots) {
    const size_t count = (size_t)N * N * N;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t sz = (size_t)N, sx = (size_t)N * N;
    EditReport report;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const unsigned own = lab[i];
        if (label_solid(own) && label_kept(own)) continue;
        const float stored = dense[i];
        const float d = vrt_grid::decode(stored, TEXEL16);
        const int y = (int)(i % sz);
        const size_t row = i / sz;
        const int x = (int)(row / sz), z = (int)(row % sz);
        if (label_solid(own)) {
            const float m = removed_density(d, gap);
            dense[i] = TEXEL16 ? vrt_grid::texel16_value(m) : m;
            if (material_id >= 0) material[i] = (uint8_t)material_id;
            report.add(N, x, y, z, true);
            continue;
        }
        if (!halo_candidate(d, gap)) continue;
        bool removed = false, kept = false;
        const auto look = [&](bool there, size_t at) {
            if (!there) return;
            const unsigned nb = lab[at];
            removed = removed || label_removed(nb);
            kept = kept || label_kept(nb);
        };
        look(y > 0, i - 1), look(y + 1 < N, i + 1);
        look(z > 0, i - sz), look(z + 1 < N, i + sz);
        look(x > 0, i - sx), look(x + 1 < N, i + sx);
        if (!removed || kept) continue;
        const float value = TEXEL16 ? vrt_grid::texel16_value(gap) : gap;
        if (__float_as_uint(value) == __float_as_uint(stored)) continue;
        dense[i] = value;
        report.add(N, x, y, z, true);
    }
    report.commit(slots, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
}

unsigned* header_of(void* scratch) { return static_cast<unsigned*>(scratch); }
unsigned* labels_of(void* scratch) { return reinterpret_cast<unsigned*>(static_cast<char*>(scratch) + kHeaderBytes); }
unsigned* rows_of(void* scratch, int N) { return labels_of(scratch) + (size_t)N * N * N; }
unsigned stride_grid(size_t count, size_t most) { return (unsigned)std::max<size_t>(1, std::min<size_t>((count + 255) / 256, most)); }

/* scratch: components_scratch_bytes(N) of device memory — a header of counters and two
   words per sample: the labels (components_core.h) and, at every root's key, its row in the table —, valid from
   launch_components_label to launch_components_apply.  table: components_table_bytes(components) of device memory, 32 B a component. */
size_t components_scratch_bytes(int N) { return kHeaderBytes + 2 * sizeof(unsigned) * (size_t)N * N * N; }
size_t components_table_bytes(unsigned components) { return std::max<size_t>(1, components) * sizeof(DComponent); }
/* device memory: the labels, one word per sample in the grid's own order, every solid sample's the lowest key of its component
   once launch_components_label has run; the header's words {gave up, components} */
const unsigned* components_labels(const void* scratch) { return labels_of(const_cast<void*>(scratch)); }
const unsigned* components_header(const void* scratch) { return header_of(const_cast<void*>(scratch)); }

/* Labels every sample: the tiles on their own, the union of what meets across tile faces, every label made its root; counts the
   roots.  A find or a union that ran into its cap leaves the header's first word non-zero. */
hipError_t launch_components_label(const float* dense, bool texel16, int N, void* scratch, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(scratch, 0, kHeaderBytes, stream);
    if (e != hipSuccess) return e;
    const size_t count = (size_t)N * N * N;
    const unsigned T = (unsigned)vrt_fill::row_bytes(N);
    hipLaunchKernelGGL(components_local_kernel, dim3(T, T, T), dim3(64), 0, stream, dense, (int)texel16, N, labels_of(scratch));
    hipLaunchKernelGGL(components_merge_kernel, dim3(stride_grid(count, 1u << 16)), dim3(256), 0, stream, N, labels_of(scratch), header_of(scratch));
    hipLaunchKernelGGL(components_flatten_kernel, dim3(stride_grid(count, 1u << 16)), dim3(256), 0, stream, N, labels_of(scratch),
                       header_of(scratch));
    return hipGetLastError();
}

/* One row of the table per component, in no particular order: its key, its samples and their box; `components`: the header's count. */
hipError_t launch_components_stats(int N, void* scratch, void* table, unsigned components, hipStream_t stream) {
    const size_t count = (size_t)N * N * N;
    hipLaunchKernelGGL(components_roots_kernel, dim3(stride_grid(count, 1u << 16)), dim3(256), 0, stream, N, labels_of(scratch), rows_of(scratch, N),
                       static_cast<DComponent*>(table), components, header_of(scratch));
    /* few waves, long loops: a large component's lanes meet at its row only once each */
    hipLaunchKernelGGL(components_stats_kernel, dim3(stride_grid(count, 2048)), dim3(256), 0, stream, N, labels_of(scratch), rows_of(scratch, N),
                       static_cast<DComponent*>(table));
    return hipGetLastError();
}

/* Row `row` of a host copy of the table. */
void components_decode_row(const void* table, size_t row, int N, vrt_components_core::Component& out) {
    const DComponent& c = static_cast<const DComponent*>(table)[row];
    out.key = c.key;
    out.samples = c.samples;
    for (int a = 0; a < 3; a++) out.lo[a] = N - (int)c.inv_lo[a], out.hi[a] = (int)c.hi1[a] - 1;
}

/* The samples of every component the predicate removes (mode, a, b: components_core.h, removed_by) store removed_density (its texel
   when texel16) and, material_id >= 0, that id; their halo stores the gap.  slots: zeroed, then the written samples' counts and box
   (the edit report, vrt_launch.h).  The labels are spent afterwards. */
hipError_t launch_components_apply(bool texel16, float* dense, uint8_t* material, int N, void* scratch, const void* table, int mode, unsigned a,
                                   unsigned b, float gap, int material_id, DBrushSlot* slots, hipStream_t stream) {
    hipError_t e = clear_report(slots, stream);
    if (e != hipSuccess) return e;
    const size_t count = (size_t)N * N * N;
    const unsigned grid = stride_grid(count, 1u << 16);
    hipLaunchKernelGGL(components_mark_kernel, dim3(grid), dim3(256), 0, stream, N, labels_of(scratch), rows_of(scratch, N),
                       static_cast<const DComponent*>(table), mode, a, b);
    if (texel16)
        hipLaunchKernelGGL(components_apply_kernel<true>, dim3(grid), dim3(256), 0, stream, dense, material, N, labels_of(scratch), gap, material_id,
                           slots);
    else
        hipLaunchKernelGGL(components_apply_kernel<false>, dim3(grid), dim3(256), 0, stream, dense, material, N, labels_of(scratch), gap,
                           material_id, slots);
    return hipGetLastError();
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_components) == 64 && sizeof(vrt_component) == 48 && sizeof(vrt_components_result) == 64, "vrt.h states these sizes");

extern "C" {

/* vrt_volume_components: first every device gets its label memory; then every device labels its copy (launch_components_label),
 * reports how many components it found, gets its table and fills it (launch_components_stats) — the volume is still untouched.
 * Device 0's table, sorted, is the list; it and (seed ops) the labels around the seed decide the removal predicate, which is the
 * same mode and scalars on every device.  Only then, and only when something goes, the edit runs per device
 * (launch_components_apply, which reports like a brush launch) and what the slot derives from the samples is recomputed over the
 * written box (rebuild_derived).  Afterwards every buffer equals what upload_volume builds from the edited volume. */
int vrt_volume_components(vrt_ctx* ctx, int slot, const vrt_components* rec, vrt_component* list, int list_capacity, vrt_components_result* result) {
    namespace cc = vrt_components_core;
    if (!ctx || !rec) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    HostVolume& h = ctx->vol[slot];
    const int N = h.N;
    const bool texel16 = h.format == VRT_FORMAT_TEXEL16;
    if (!cc::valid(rec, N, texel16, list, list_capacity)) return VRT_ERR_INVALID;
    vrt_components_result out;
    memset(&out, 0, sizeof out);
    for (int a = 0; a < 3; a++) out.lo[a] = N, out.hi[a] = -1;
    int rc = quiesce(ctx);
    if (rc != VRT_OK) return rc;
    for (auto& D : ctx->dev) { /* the read phase allocates all the call needs: its run_edit has nothing left to prepare */
        HIP_TRY(hipSetDevice(D.ordinal));
        rc = ensure_buffer(D.buf[kBufCompLabels], components_scratch_bytes(N));
        if (rc != VRT_OK) return rc;
    }
    unsigned n_components = 0;
    for (size_t di = 0; di < ctx->dev.size(); di++) {
        DeviceState& D = ctx->dev[di];
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(launch_components_label(D.vol[slot].dense, texel16, N, D.buf[kBufCompLabels].p, D.stream));
        unsigned header[2];
        HIP_TRY(hipMemcpyAsync(header, components_header(D.buf[kBufCompLabels].p), sizeof header, hipMemcpyDeviceToHost, D.stream));
        HIP_TRY(hipStreamSynchronize(D.stream));
        if (header[0] != 0u || (di > 0 && header[1] != n_components)) {
            fprintf(stderr, "[vrt] vrt_volume_components: the labelling of a grid of %d^3 gave up on device %d\n", N, D.ordinal);
            return VRT_ERR_HIP;
        }
        n_components = header[1];
        rc = ensure_buffer(D.buf[kBufCompTable], components_table_bytes(n_components));
        if (rc != VRT_OK) return rc;
        if (n_components > 0) HIP_TRY(launch_components_stats(N, D.buf[kBufCompLabels].p, D.buf[kBufCompTable].p, n_components, D.stream));
    }
    std::vector<cc::Component> comps(n_components);
    cc::Decision how;
    if (n_components > 0) {
        DeviceState& D0 = ctx->dev[0];
        HIP_TRY(hipSetDevice(D0.ordinal));
        std::vector<unsigned char> raw(components_table_bytes(n_components));
        HIP_TRY(hipMemcpyAsync(raw.data(), D0.buf[kBufCompTable].p, raw.size(), hipMemcpyDeviceToHost, D0.stream));
        unsigned gave_up = 0;
        HIP_TRY(hipMemcpyAsync(&gave_up, components_header(D0.buf[kBufCompLabels].p), sizeof gave_up, hipMemcpyDeviceToHost, D0.stream));
        HIP_TRY(hipStreamSynchronize(D0.stream));
        if (gave_up != 0u) return VRT_ERR_HIP;
        for (size_t i = 0; i < comps.size(); i++) components_decode_row(raw.data(), i, N, comps[i]);
        std::sort(comps.begin(), comps.end(), cc::before);
    }
    uint32_t seed_label = cc::kPassable;
    if (cc::seeded(rec->op)) { /* the labels of the seed's neighbourhood: up to nine runs of three along y */
        uint32_t around[3][3][3];
        for (auto& plane : around)
            for (auto& line : plane)
                for (uint32_t& l : line) l = cc::kPassable;
        DeviceState& D0 = ctx->dev[0];
        HIP_TRY(hipSetDevice(D0.ordinal));
        const int y0 = std::max(rec->seed[1] - 1, 0), y1 = std::min(rec->seed[1] + 1, N - 1);
        for (int dx = -1; dx <= 1; dx++)
            for (int dz = -1; dz <= 1; dz++) {
                const int x = rec->seed[0] + dx, z = rec->seed[2] + dz;
                if (x < 0 || z < 0 || x >= N || z >= N) continue;
                HIP_TRY(hipMemcpyAsync(&around[dx + 1][dz + 1][y0 - rec->seed[1] + 1], components_labels(D0.buf[kBufCompLabels].p) + cc::key_of(N, x, y0, z),
                                       (size_t)(y1 - y0 + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, D0.stream));
            }
        HIP_TRY(hipStreamSynchronize(D0.stream));
        seed_label = cc::seed_component(N, rec->seed, [&](int x, int y, int z) {
            return around[x - rec->seed[0] + 1][z - rec->seed[2] + 1][y - rec->seed[1] + 1];
        });
    }
    if (!cc::decide(*rec, comps.data(), comps.size(), seed_label, how)) return VRT_ERR_INVALID; /* nothing has been written */
    out.components = n_components;
    for (size_t i = 0; i < comps.size(); i++) {
        const cc::Component& c = comps[i];
        const bool goes = cc::removes(rec->op) && cc::removed_by(how.mode, how.a, how.b, c.key, c.samples);
        out.solid += c.samples;
        if (goes) out.removed++, out.removed_samples += c.samples;
        if (i < (size_t)list_capacity) {
            vrt_component& r = list[i];
            memset(&r, 0, sizeof r);
            cc::first_of(N, c.key, r.first);
            for (int a = 0; a < 3; a++) r.lo[a] = c.lo[a], r.hi[a] = c.hi[a];
            r.removed = goes ? 1u : 0u;
            r.samples = c.samples;
            out.listed++;
        }
    }
    if (out.removed > 0) { /* only a call that removes something is an edit; its footprint is the whole grid */
        const int zero[3] = {0, 0, 0}, last[3] = {N - 1, N - 1, N - 1};
        Edit e;
        e.slot = slot;
        e.foot = derived_boxes(h, zero, last).samples;
        e.rebuild = Edit::kWrites; /* every written sample is a density write */
        e.write = [&](DeviceState& D, size_t) -> int {
            DeviceVolume& v = D.vol[slot];
            HIP_TRY(launch_components_apply(texel16, v.dense, v.material, N, D.buf[kBufCompLabels].p, D.buf[kBufCompTable].p, how.mode, how.a, how.b,
                                            rec->gap, rec->material, D.d_brush, D.stream));
            return VRT_OK;
        };
        e.reported = [&](const Written& got) {
            for (int a = 0; a < 3; a++) out.lo[a] = got.lo[a], out.hi[a] = got.hi[a];
            out.written = got.low;
        };
        if ((rc = run_edit(ctx, e)) != VRT_OK) return rc;
    }
    if (result) *result = out;
    return VRT_OK;
}

}  // extern "C"
