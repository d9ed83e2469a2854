/* vrt_mask.hip — vrt_volume_mask_apply, _upload, _download, _clear and _info (include/vrt.h), kernels to driver, and the mask's share of
 * run_edit (mask_put_back, vrt_context.h): a slot's protected samples, one bit each in mask_core.h's layout — a row of N samples along
 * y is ceil(N / 64) words, which is what a wave of 64 lanes along y produces with one ballot.  Eight kernels.  The records' kernels
 * (predicate, invert, grow, shrink) change the mask and read the volume; put-back, after an honouring edit, gives the protected
 * samples of the call's footprint the bits the history's capture kernel copied aside (kBufHistory: one copy serves both); count finds
 * the set bits' number and box for the host's books; pack and unpack move a mask between bytes and words.  Nothing here reads a
 * density as a float but SOLID's test. */
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>

#include "mask_core.h"
#include "vrt_context.h"

namespace vrt {

namespace M = vrt_mask_core;

/* A record as the predicate kernel reads it: the fields of a vrt_mask_op that select, and the slot's format. */
struct DMaskOp {
    int32_t kind, value, shape;
    float a[3], b[3], radius;
    int32_t material;
    int32_t texel16;
};

/* What the count kernel leaves (device memory, zeroed ahead of it): every field grows from 0 = no set bit, as an edit report's. */
struct DMaskCount {
    unsigned long long masked;
    uint32_t inv_lo[3]; /* N - lowest x, y, z */
    uint32_t hi1[3];    /* 1 + highest x, y, z */
    uint32_t pad_[8];
};
static_assert(sizeof(DMaskCount) == 64, "the count record heads the scratch buffer");

/* One wave per word of the word box `words` ({x, z, word of the row}), lane l at sample y = 64 j + l: the ballot of the record's
 * predicate is the word of selected bits, and lane 0, the word's only writer, sets or clears them.  Lanes past the row's end select
 * nothing, so the tail bits stay 0.  Only the kinds that ask for them load a density or an id. */
__global__ __launch_bounds__(256) void mask_predicate_kernel(DMaskOp op, const float* __restrict__ dense, const uint8_t* __restrict__ material,
                                                             int N, EditBox words, unsigned n_words, uint64_t* __restrict__ mask) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= n_words) return; /* the whole wave */
    int x, z, j;
    box_coords(words, (size_t)w, x, z, j);
    const int y = j * 64 + (int)lane;
    bool sel = false;
    if (y < N) {
        const size_t g = vrt_grid::index(N, x, y, z);
        const float stored = op.kind == VRT_MASK_SOLID ? dense[g] : 0.0f;
        const unsigned id = op.kind == VRT_MASK_MATERIAL ? material[g] : 0u;
        sel = M::selects(op, x, y, z, stored, id, op.texel16 != 0);
    }
    const uint64_t bits = __ballot(sel);
    if (lane == 0u) {
        const size_t at = M::word_index(N, x, z, j);
        mask[at] = M::assign(mask[at], bits, op.value);
    }
}

/* One lane per word: every live bit flips. */
__global__ __launch_bounds__(256) void mask_invert_kernel(uint64_t* __restrict__ mask, int N, size_t n_words) {
    const int W = M::row_words(N);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride) mask[i] ^= M::live_bits(N, (int)(i % (size_t)W));
}

/* One step of GROW (SHRINK false) or SHRINK, one lane per word, from `in` into `out` (never the same buffer): the word with its bits
 * moved one sample either way along y — the carries come from the row's neighbouring words — and the same word of the four
 * neighbouring rows (mask_core.h).  Words beyond the grid read as 0, after SHRINK's complement as before it. */
template <bool SHRINK>
__global__ __launch_bounds__(256) void mask_grow_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int N, size_t n_words) {
    const int W = M::row_words(N);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride) {
        const int j = (int)(i % (size_t)W);
        const size_t row = i / (size_t)W;
        const int z = (int)(row % (size_t)N), x = (int)(row / (size_t)N);
        const auto word = [&](int wx, int wz, int wj) -> uint64_t {
            if (wx < 0 || wx >= N || wz < 0 || wz >= N || wj < 0 || wj >= W) return 0ull;
            const uint64_t v = in[M::word_index(N, wx, wz, wj)];
            return SHRINK ? M::shrink_in(v, M::live_bits(N, wj)) : v;
        };
        const uint64_t live = M::live_bits(N, j);
        const uint64_t grown = M::grow_word(word(x, z, j), word(x, z, j - 1), word(x, z, j + 1), word(x - 1, z, j), word(x + 1, z, j),
                                            word(x, z - 1, j), word(x, z + 1, j), live);
        out[i] = SHRINK ? M::shrink_out(grown, live) : grown;
    }
}

/* After an honouring edit: a wave per word of the word box `words`, which covers the copied box `foot` (samples, {x, z, y}); the launch
 * is capped, and a wave walks on to further words, so that the waves' counts meet in few atomics on one counter.  A word without a set
 * bit costs its wave one uniform load.  A lane whose bit is set and whose sample lies in `foot` compares the sample's stored bits and id
 * with the copy and writes back what differs; at its end the wave adds its count of such samples to *restored. */
__global__ __launch_bounds__(256) void mask_put_back_kernel(const uint64_t* __restrict__ mask, int N, EditBox words, unsigned n_words,
                                                            EditBox foot, const uint32_t* __restrict__ pre_bits,
                                                            const uint8_t* __restrict__ pre_ids, uint32_t* __restrict__ dense,
                                                            uint8_t* __restrict__ material, unsigned long long* __restrict__ restored) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned waves = gridDim.x * (blockDim.x >> 6);
    unsigned n = 0u; /* the same in every lane */
    for (unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_words; w += waves) { /* the whole wave */
        int x, z, j;
        box_coords(words, (size_t)w, x, z, j);
        const uint64_t word = mask[M::word_index(N, x, z, j)];
        if (word == 0ull) continue; /* the whole wave */
        const int y = j * 64 + (int)lane;
        bool differs = false;
        if (((word >> lane) & 1ull) != 0ull && y >= foot.lo[2] && y < foot.lo[2] + foot.n[2]) { /* a set bit is a sample of the grid */
            const size_t g = vrt_grid::index(N, x, y, z);
            const size_t i = box_index(foot, x, z, y);
            const uint32_t was_bits = pre_bits[i], now_bits = dense[g];
            const unsigned was_id = pre_ids[i], now_id = material[g];
            if (now_bits != was_bits) dense[g] = was_bits;
            if (now_id != was_id) material[g] = (uint8_t)was_id;
            differs = now_bits != was_bits || now_id != was_id;
        }
        n += (unsigned)__popcll(__ballot(differs));
    }
    if (lane == 0u && n != 0u) atomicAdd(restored, (unsigned long long)n);
}

/* The set bits' number and box, one lane per word: a lane keeps its words' sums, the wave folds them, and lane 0 of a wave that saw a
 * set bit adds them to the record with one atomic per field. */
__global__ __launch_bounds__(256) void mask_count_kernel(const uint64_t* __restrict__ mask, int N, size_t n_words, DMaskCount* __restrict__ out) {
    const int W = M::row_words(N);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    unsigned n = 0u, inv_lo_x = 0u, inv_lo_y = 0u, inv_lo_z = 0u, hi1_x = 0u, hi1_y = 0u, hi1_z = 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride) {
        const uint64_t word = mask[i];
        if (word == 0ull) continue;
        const int j = (int)(i % (size_t)W);
        const size_t row = i / (size_t)W;
        const int z = (int)(row % (size_t)N), x = (int)(row / (size_t)N);
        const int y_lo = j * 64 + (__ffsll((unsigned long long)word) - 1), y_hi = j * 64 + 63 - __clzll((long long)word);
        n += (unsigned)__popcll(word);
        inv_lo_x = max(inv_lo_x, (unsigned)(N - x)), inv_lo_y = max(inv_lo_y, (unsigned)(N - y_lo)), inv_lo_z = max(inv_lo_z, (unsigned)(N - z));
        hi1_x = max(hi1_x, (unsigned)(x + 1)), hi1_y = max(hi1_y, (unsigned)(y_hi + 1)), hi1_z = max(hi1_z, (unsigned)(z + 1));
    }
    for (int o = 32; o > 0; o >>= 1) {
        n += __shfl_xor(n, o);
        inv_lo_x = max(inv_lo_x, __shfl_xor(inv_lo_x, o)), inv_lo_y = max(inv_lo_y, __shfl_xor(inv_lo_y, o));
        inv_lo_z = max(inv_lo_z, __shfl_xor(inv_lo_z, o));
        hi1_x = max(hi1_x, __shfl_xor(hi1_x, o)), hi1_y = max(hi1_y, __shfl_xor(hi1_y, o)), hi1_z = max(hi1_z, __shfl_xor(hi1_z, o));
    }
    if ((threadIdx.x & 63u) != 0u || n == 0u) return;
    atomicAdd(&out->masked, (unsigned long long)n);
    atomicMax(&out->inv_lo[0], inv_lo_x), atomicMax(&out->inv_lo[1], inv_lo_y), atomicMax(&out->inv_lo[2], inv_lo_z);
    atomicMax(&out->hi1[0], hi1_x), atomicMax(&out->hi1[1], hi1_y), atomicMax(&out->hi1[2], hi1_z);
}

/* Bytes in grid order to words and back, one wave per word of the grid, lane l at sample y = 64 j + l. */
__global__ __launch_bounds__(256) void mask_pack_kernel(const uint8_t* __restrict__ bytes, int N, unsigned n_words, uint64_t* __restrict__ mask) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= n_words) return; /* the whole wave */
    const int W = M::row_words(N);
    const int j = (int)(w % (unsigned)W), y = j * 64 + (int)lane;
    const size_t row = w / (unsigned)W; /* x * N + z */
    const uint64_t bits = __ballot(y < N && bytes[row * (size_t)N + (size_t)y] != 0);
    if (lane == 0u) mask[w] = bits;
}
__global__ __launch_bounds__(256) void mask_unpack_kernel(const uint64_t* __restrict__ mask, int N, unsigned n_words, uint8_t* __restrict__ bytes) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= n_words) return; /* the whole wave */
    const int W = M::row_words(N);
    const int j = (int)(w % (unsigned)W), y = j * 64 + (int)lane;
    const size_t row = w / (unsigned)W;
    if (y < N) bytes[row * (size_t)N + (size_t)y] = (uint8_t)((mask[w] >> lane) & 1ull);
}

namespace {

unsigned wave_blocks(size_t waves) { return (unsigned)((waves + 3) / 4); }
constexpr unsigned kPutBackBlocks = 2048; /* 8192 waves: every wave slot of the device, and as many adds to the put-back's counter */
unsigned lane_blocks(size_t lanes) { return (unsigned)std::min<size_t>((lanes + 255) / 256, 1u << 16); }

/* The scratch buffer (kBufMask): the count record, then what the call asks for — GROW's second copy of the mask, or N^3 staged bytes. */
size_t mask_scratch_bytes(size_t body) { return sizeof(DMaskCount) + body; }
size_t mask_copy_bytes(int N) { return M::word_count(N) * sizeof(uint64_t); }
size_t mask_staged_bytes(int N) { return (size_t)N * N * N; }
DMaskCount* count_of(void* scratch) { return static_cast<DMaskCount*>(scratch); }
void* body_of(void* scratch) { return static_cast<char*>(scratch) + sizeof(DMaskCount); }

/* The words that hold the samples of a sample box: {x, z, word of the row}. */
EditBox word_box(const EditBox& samples) {
    EditBox w = samples;
    w.lo[2] = samples.lo[2] >> 6;
    w.n[2] = ((samples.lo[2] + samples.n[2] - 1) >> 6) - w.lo[2] + 1;
    return w;
}

/* Everything a call that writes the mask may run out of, on every device, ahead of its first write: the scratch buffer with `body` bytes
 * after its count record and, for a slot without a mask, a mask of zeros.  A failure frees the masks it had allocated: the slot is as it
 * was. */
int prepare_mask(vrt_ctx* ctx, int slot, size_t body) {
    const int N = ctx->vol[slot].N;
    HostMask& hm = ctx->mask[slot];
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        int rc = ensure_buffer(D.buf[kBufMask], mask_scratch_bytes(body));
        if (rc != VRT_OK) return rc;
    }
    if (hm.on) return VRT_OK;
    const size_t bytes = M::word_count(N) * sizeof(uint64_t);
    hipError_t e = hipSuccess;
    for (auto& D : ctx->dev) {
        if ((e = hipSetDevice(D.ordinal)) != hipSuccess) break;
        if ((e = hipMalloc(&D.vol[slot].mask, bytes)) != hipSuccess) {
            D.vol[slot].mask = nullptr;
            break;
        }
        if ((e = hipMemsetAsync(D.vol[slot].mask, 0, bytes, D.stream)) != hipSuccess) break;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (auto& D : ctx->dev) {
            if (!D.vol[slot].mask || hipSetDevice(D.ordinal) != hipSuccess) continue;
            (void)hipStreamSynchronize(D.stream);
            (void)hipFree(D.vol[slot].mask);
            D.vol[slot].mask = nullptr;
        }
        return e == hipErrorOutOfMemory ? VRT_ERR_OOM : VRT_ERR_HIP;
    }
    hm = HostMask();
    hm.on = true;
    for (int a = 0; a < 3; a++) hm.lo[a] = N;
    return VRT_OK;
}

/* One record on one device, after whatever the stream holds. */
hipError_t launch_mask_op(const vrt_mask_op& r, const HostVolume& h, const DeviceVolume& v, void* scratch, hipStream_t stream) {
    const int N = h.N;
    const size_t n_words = M::word_count(N);
    if (r.kind == VRT_MASK_INVERT) {
        hipLaunchKernelGGL(mask_invert_kernel, dim3(lane_blocks(n_words)), dim3(256), 0, stream, v.mask, N, n_words);
        return hipGetLastError();
    }
    if (r.kind == VRT_MASK_GROW || r.kind == VRT_MASK_SHRINK) {
        uint64_t* buf[2] = {v.mask, static_cast<uint64_t*>(body_of(scratch))};
        for (int s = 0; s < r.steps; s++) {
            if (r.kind == VRT_MASK_GROW)
                hipLaunchKernelGGL(mask_grow_kernel<false>, dim3(lane_blocks(n_words)), dim3(256), 0, stream, buf[s & 1], buf[(s + 1) & 1], N, n_words);
            else
                hipLaunchKernelGGL(mask_grow_kernel<true>, dim3(lane_blocks(n_words)), dim3(256), 0, stream, buf[s & 1], buf[(s + 1) & 1], N, n_words);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && (r.steps & 1)) e = hipMemcpyAsync(buf[0], buf[1], n_words * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream);
        return e;
    }
    /* the selecting kinds: over the whole grid, or (SHAPE) over the words that hold the shape's box */
    EditBox words = {{0, 0, 0}, {N, N, M::row_words(N)}};
    if (r.kind == VRT_MASK_SHAPE) {
        int lo[3], hi[3];
        if (!M::shape_box(r, N, lo, hi)) return hipSuccess; /* wholly outside the grid */
        words = word_box(derived_boxes(h, lo, hi).samples);
    }
    DMaskOp op;
    memset(&op, 0, sizeof op);
    op.kind = r.kind, op.value = r.value, op.shape = r.shape;
    memcpy(op.a, r.a, sizeof op.a);
    memcpy(op.b, r.b, sizeof op.b);
    op.radius = r.radius;
    op.material = r.material;
    op.texel16 = h.format == VRT_FORMAT_TEXEL16 ? 1 : 0;
    const size_t n = box_count(words);
    hipLaunchKernelGGL(mask_predicate_kernel, dim3(wave_blocks(n)), dim3(256), 0, stream, op, v.dense, v.material, N, words, (unsigned)n, v.mask);
    return hipGetLastError();
}

/* After a call that wrote the mask: device 0 counts for the host's books, and every device's stream has run dry. */
int count_mask(vrt_ctx* ctx, int slot) {
    const int N = ctx->vol[slot].N;
    HostMask& hm = ctx->mask[slot];
    DeviceState& D0 = ctx->dev[0];
    DMaskCount got;
    HIP_TRY(hipSetDevice(D0.ordinal));
    DMaskCount* d_count = count_of(D0.buf[kBufMask].p);
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof got, D0.stream));
    hipLaunchKernelGGL(mask_count_kernel, dim3(lane_blocks(M::word_count(N))), dim3(256), 0, D0.stream, D0.vol[slot].mask, N, M::word_count(N), d_count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&got, d_count, sizeof got, hipMemcpyDeviceToHost, D0.stream));
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipStreamSynchronize(D.stream));
    }
    hm.masked = got.masked;
    for (int a = 0; a < 3; a++) {
        hm.lo[a] = N - (int)got.inv_lo[a];
        hm.hi[a] = (int)got.hi1[a] - 1;
    }
    return VRT_OK;
}

void fill_info(const vrt_ctx* ctx, int slot, vrt_mask_info* out) {
    const HostMask& hm = ctx->mask[slot];
    const int N = ctx->vol[slot].N;
    *out = vrt_mask_info{};
    out->on = hm.on ? 1 : 0;
    out->masked = hm.masked;
    for (int a = 0; a < 3; a++) {
        out->lo[a] = hm.masked > 0 ? hm.lo[a] : N;
        out->hi[a] = hm.masked > 0 ? hm.hi[a] : -1;
    }
    out->restored = hm.restored;
}

}  // namespace

/* ---- The mask's share of run_edit ---- */
int mask_put_back(vrt_ctx* ctx, size_t di, int slot, const HistoryCall& call) {
    if (!call.captured || !call.protects) return VRT_OK;
    DeviceState& D = ctx->dev[di];
    const DeviceVolume& v = D.vol[slot];
    HostMask& hm = ctx->mask[slot];
    const int N = ctx->vol[slot].N;
    /* the words to walk: those of the copied box that the set bits' box meets (the copy is the whole footprint when the history asked) */
    EditBox area = call.foot;
    for (int a = 0; a < 3; a++) {
        const int lo = std::max(call.foot.lo[a], hm.lo[grid_axis(a)]), hi = std::min(call.foot.lo[a] + call.foot.n[a] - 1, hm.hi[grid_axis(a)]);
        if (lo > hi) return VRT_OK; /* nothing protected in the footprint: `restored` stays 0 */
        area.lo[a] = lo;
        area.n[a] = hi - lo + 1;
    }
    const EditBox words = word_box(area);
    const size_t n = box_count(words);
    const CaptureView copy = capture_view(D.buf[kBufHistory].p, box_count(call.foot));
    hipLaunchKernelGGL(mask_put_back_kernel, dim3(std::min(wave_blocks(n), kPutBackBlocks)), dim3(256), 0, D.stream, v.mask, N, words,
                       (unsigned)n, call.foot, copy.bits, copy.ids, reinterpret_cast<uint32_t*>(v.dense), v.material, copy.restored);
    HIP_TRY(hipGetLastError());
    static_assert(sizeof hm.restored == sizeof(unsigned long long), "the counter is copied as it is");
    if (di == 0) HIP_TRY(hipMemcpyAsync(&hm.restored, copy.restored, sizeof hm.restored, hipMemcpyDeviceToHost, D.stream));
    return VRT_OK;
}

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_mask_op) == 64 && sizeof(vrt_mask_info) == 48, "vrt.h states these sizes");
static_assert(sizeof(DMaskOp) <= 64, "a record travels in the kernel-argument block");

extern "C" {

int vrt_volume_mask_apply(vrt_ctx* ctx, int slot, int n, const vrt_mask_op* ops, vrt_mask_info* info_or_null) {
    if (!ctx || !M::valid_mask_ops(n, ops)) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    const HostVolume& h = ctx->vol[slot];
    bool steps = false; /* only GROW and SHRINK need a second copy of the mask */
    for (int i = 0; i < n; i++) steps = steps || ops[i].kind == VRT_MASK_GROW || ops[i].kind == VRT_MASK_SHRINK;
    int rc = quiesce(ctx);
    if (rc == VRT_OK) rc = prepare_mask(ctx, slot, steps ? mask_copy_bytes(h.N) : 0);
    if (rc != VRT_OK) return rc;
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        for (int i = 0; i < n; i++) HIP_TRY(launch_mask_op(ops[i], h, D.vol[slot], D.buf[kBufMask].p, D.stream));
    }
    if ((rc = count_mask(ctx, slot)) != VRT_OK) return rc;
    if (info_or_null) fill_info(ctx, slot, info_or_null);
    return VRT_OK;
}

int vrt_volume_mask_upload(vrt_ctx* ctx, int slot, const uint8_t* bytes) {
    if (!ctx || !bytes) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    const int N = ctx->vol[slot].N;
    int rc = quiesce(ctx);
    if (rc == VRT_OK) rc = prepare_mask(ctx, slot, mask_staged_bytes(N));
    if (rc != VRT_OK) return rc;
    const size_t count = (size_t)N * N * N, n_words = M::word_count(N);
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        uint8_t* staged = static_cast<uint8_t*>(body_of(D.buf[kBufMask].p));
        HIP_TRY(hipMemcpyAsync(staged, bytes, count, hipMemcpyHostToDevice, D.stream));
        hipLaunchKernelGGL(mask_pack_kernel, dim3(wave_blocks(n_words)), dim3(256), 0, D.stream, staged, N, (unsigned)n_words, D.vol[slot].mask);
        HIP_TRY(hipGetLastError());
    }
    return count_mask(ctx, slot);
}

int vrt_volume_mask_download(vrt_ctx* ctx, int slot, uint8_t* out) {
    if (!ctx || !out) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    const int N = ctx->vol[slot].N;
    const size_t count = (size_t)N * N * N, n_words = M::word_count(N);
    if (!ctx->mask[slot].on) {
        memset(out, 0, count);
        return VRT_OK;
    }
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    int rc = ensure_buffer(D.buf[kBufMask], mask_scratch_bytes(mask_staged_bytes(N)));
    if (rc != VRT_OK) return rc;
    uint8_t* staged = static_cast<uint8_t*>(body_of(D.buf[kBufMask].p));
    hipLaunchKernelGGL(mask_unpack_kernel, dim3(wave_blocks(n_words)), dim3(256), 0, D.stream, D.vol[slot].mask, N, (unsigned)n_words, staged);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, staged, count, hipMemcpyDeviceToHost, D.stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    return VRT_OK;
}

int vrt_volume_mask_clear(vrt_ctx* ctx, int slot) {
    if (!ctx) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    if (!ctx->mask[slot].on) return VRT_OK;
    for (auto& D : ctx->dev) {
        HIP_TRY(hipSetDevice(D.ordinal));
        HIP_TRY(hipDeviceSynchronize());
        if (D.vol[slot].mask) HIP_TRY(hipFree(D.vol[slot].mask));
        D.vol[slot].mask = nullptr;
    }
    ctx->mask[slot] = HostMask();
    return VRT_OK;
}

int vrt_volume_mask_info(vrt_ctx* ctx, int slot, vrt_mask_info* out) {
    if (!ctx || !out) return VRT_ERR_INVALID;
    if (!valid_slot(slot) || !ctx->vol[slot].used) return VRT_ERR_SLOT;
    fill_info(ctx, slot, out);
    return VRT_OK;
}

}  // extern "C"
