/* vrt_contacts.hip — vrt_query_contacts (include/vrt.h), kernels to driver: the surface points of instance A that lie in or near
 * instance B, as compact records in the order of A's cells.  The rule is csrc/contacts_core.h over csrc/mesh_core.h.
 *
 * The mesh call's shape (vrt_mesh.hip): the unit of work is a run, 64 consecutive cells along y of one (x, z) row of the clipped cell
 * box of A, one wave, lane = cell; runs are numbered in the grid's storage order, so run order followed by lane order IS the order of
 * the cells' keys.
 *   count   every lane loads its cell's eight corners of A (y fastest: coalesced rows); the few active lanes make the vertex, take it to
 *           the world and into B, and fetch B's eight taps there — as vrt_points.hip does, four y-adjacent pairs, on the sparse active
 *           lanes as they are (DESIGN §2 has why) — and the contact test goes through __ballot into the run's 16-byte record.  The
 *           wave's candidates and its contacts' cell box leave through the edit report, the smallest distance through one atomicMin on
 *           an order-preserving key: integers all, which no order of waves can change.
 *   scan    an exclusive prefix sum over the records' counts (three launches: block sums, their scan, the records).
 *   emit    a run with a non-empty mask recomputes its contact lanes with the same inline function — the same bits — and writes each
 *           record as four 16-byte stores at first + popcount(mask below the lane).  No N^3 index volume, no atomics on the order.
 * A's and B's descriptors are wave-uniform and travel in the kernarg: they come through scalar loads. */
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <cmath>

#include "contacts_core.h"
#include "edit_report.h"
#include "vrt_context.h"

namespace vrt {

namespace {

namespace K = vrt_contacts;

constexpr int kRunsPerBlock = 4;  /* count / emit: 256 lanes, one run per wave */
constexpr int kScanThreads = 256; /* scan: each lane takes kScanItems consecutive records */
constexpr int kScanItems = 8;
constexpr size_t kHeaderBytes = 256; /* the total (8 B) and the smallest distance's key (4 B), ahead of the block sums */

typedef unsigned long long u64;
typedef unsigned cu4 __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) * cgfloat_p;

struct alignas(16) Run {
    u64 mask;       /* bit l: cell l of the run made a contact */
    unsigned first; /* count: the contacts of the run; after the scan: the number of its first one */
    unsigned pad_;
};

struct Header {
    u64 total;        /* contacts, written by the scan */
    unsigned min_key; /* contacts_core.h's distance_key of the smallest distance; kNoKey: none */
};

/* The kernarg of count and emit. */
struct DContacts {
    K::Side A, B;
    const float* dense_a;
    const uint8_t* material_a;
    const float* dense_b;
    const uint8_t* material_b;
    int lo[3], n[3]; /* the clipped cell box of A, xyz: its first cell and its cells per axis */
    int runs_y;
    unsigned n_runs;
    float margin;
    Run* runs;
    Header* header;
    DBrushSlot* slots;
    vrt_contact* out; /* emit */
    unsigned cap;
};

/* The cell of lane `lane` of run r (xyz), and whether the row of the cell box reaches that far. */
__device__ __forceinline__ bool cell_of(const DContacts& Q, unsigned r, int lane, int c[3]) {
    const unsigned ry = r % (unsigned)Q.runs_y, t = r / (unsigned)Q.runs_y;
    const int rel_y = (int)ry * 64 + lane;
    c[0] = Q.lo[0] + (int)(t / (unsigned)Q.n[2]);
    c[1] = Q.lo[1] + rel_y;
    c[2] = Q.lo[2] + (int)(t % (unsigned)Q.n[2]);
    return rel_y < Q.n[1];
}

/* The eight corner values of cell c of A at iso 0. */
__device__ __forceinline__ void load_corners(const DContacts& Q, const int c[3], float f[8]) {
    const int N = Q.A.N;
    const bool t16 = Q.A.texel16 != 0;
    const size_t i0 = vrt_grid::index(N, c[0], c[1], c[2]);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const size_t i = i0 + (size_t)(j & 1) * N * N + (size_t)((j >> 1) & 1) + (size_t)(j >> 2) * N;
        f[j] = vrt_mesh::field(vrt_grid::decode(Q.dense_a[i], t16), 0.0f);
    }
}

/* What count and emit both compute of an ACTIVE cell c of A with the corner values f: its vertex, the world point, where that falls
   in B, B's decoded taps and value.  False: no candidate (nothing but v and w is set then). */
__device__ __forceinline__ bool candidate(const DContacts& Q, const int c[3], const float f[8], vrt_mesh::Vertex& v, float w[3], K::Probe& P,
                                          float s[8], float& value) {
    v = vrt_mesh::cell_vertex(c, f);
    K::world_point(Q.A, v.p, w);
    if (!K::locate(Q.B, w, P)) return false;
    /* [x][z][y], 0 <= c <= N - 2 on every axis: all eight taps lie inside the grid; N <= 513, so a sample's index fits 32 bits */
    const unsigned n = (unsigned)Q.B.N;
    const unsigned at = ((unsigned)P.c[0] * n + (unsigned)P.c[2]) * n + (unsigned)P.c[1];
    const cgfloat_p b00 = (cgfloat_p)(Q.dense_b) + at; /* x, z */
    const cgfloat_p b01 = b00 + n, b10 = b00 + n * n, b11 = b10 + n;
    const bool t16 = Q.B.texel16 != 0;
    /* tap j = dx + 2 dy + 4 dz; the pairs along y are adjacent loads for the compiler to merge */
    s[0] = vrt_grid::decode(b00[0], t16), s[2] = vrt_grid::decode(b00[1], t16);
    s[4] = vrt_grid::decode(b01[0], t16), s[6] = vrt_grid::decode(b01[1], t16);
    s[1] = vrt_grid::decode(b10[0], t16), s[3] = vrt_grid::decode(b10[1], t16);
    s[5] = vrt_grid::decode(b11[0], t16), s[7] = vrt_grid::decode(b11[1], t16);
    return K::value_at(Q.B, P, s, value);
}

__global__ __launch_bounds__(256) void contacts_count_kernel(const DContacts Q) {
    const unsigned r = blockIdx.x * kRunsPerBlock + (threadIdx.x >> 6);
    if (r >= Q.n_runs) return; /* the whole wave */
    const int lane = (int)(threadIdx.x & 63u);
    int c[3];
    bool cand = false, hit = false;
    float value = 0.0f;
    if (cell_of(Q, r, lane, c)) {
        float f[8];
        load_corners(Q, c, f);
        if (vrt_mesh::active(vrt_mesh::corner_classes(f))) {
            vrt_mesh::Vertex v;
            K::Probe P;
            float w[3], s[8];
            cand = candidate(Q, c, f, v, w, P, s, value);
            hit = cand && value <= Q.margin;
        }
    }
    const u64 mask = __ballot(hit), cands = __ballot(cand);
    unsigned key = hit ? K::distance_key(value) : K::kNoKey;
    if (mask != 0ull) { /* wave-uniform */
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o));
    }
    if (lane != 0) return;
    Run rec;
    rec.mask = mask, rec.first = (unsigned)__popcll(mask), rec.pad_ = 0u;
    Q.runs[r] = rec;
    if (cands == 0ull) return;
    EditReport report;
    report.n_low = report.n_low_only = (unsigned)__popcll(cands); /* the candidates: the low half of `counts` */
    if (mask != 0ull) { /* lane 0's cell is the run's first: x and z are the run's, y runs from the lowest to the highest set bit */
        const int y_lo = c[1] + (int)__ffsll((long long)mask) - 1, y_hi = c[1] + 63 - (int)__clzll((long long)mask);
        report.bound(Q.A.N, c[0], y_lo, c[2]);
        report.bound(Q.A.N, c[0], y_hi, c[2]);
        atomicMin(&Q.header->min_key, key);
    }
    report.write(Q.slots, r);
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
__global__ __launch_bounds__(kScanThreads) void contacts_scan_reduce_kernel(const Run* __restrict__ runs, unsigned n_runs, u64* __restrict__ sums) {
    __shared__ u64 wave_sum[kScanThreads / 64];
    const size_t first = ((size_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
    u64 mine = 0ull;
#pragma unroll
    for (int j = 0; j < kScanItems; j++)
        if (first + j < n_runs) mine += runs[first + j].first;
    u64 total;
    (void)block_exclusive_scan(mine, total, wave_sum);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

/* One workgroup: sums -> their exclusive prefix sums, *total = the sum of all. */
__global__ __launch_bounds__(kScanThreads) void contacts_scan_sums_kernel(u64* __restrict__ sums, unsigned n_blocks, u64* __restrict__ total_out) {
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
    if (threadIdx.x == 0) *total_out = carry;
}

/* The records' counts -> the runs' first contact. */
__global__ __launch_bounds__(kScanThreads) void contacts_scan_apply_kernel(Run* __restrict__ runs, unsigned n_runs, const u64* __restrict__ sums) {
    __shared__ u64 wave_sum[kScanThreads / 64];
    const size_t first = ((size_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
    unsigned count[kScanItems];
    u64 mine = 0ull;
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        count[j] = first + j < n_runs ? runs[first + j].first : 0u;
        mine += count[j];
    }
    u64 total;
    u64 at = sums[blockIdx.x] + block_exclusive_scan(mine, total, wave_sum);
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        if (first + j < n_runs) runs[first + j].first = (unsigned)at;
        at += count[j];
    }
}

__global__ __launch_bounds__(256) void contacts_emit_kernel(const DContacts Q) {
    const unsigned r = blockIdx.x * kRunsPerBlock + (threadIdx.x >> 6);
    if (r >= Q.n_runs) return; /* the whole wave */
    const Run rec = Q.runs[r];
    if (rec.mask == 0ull) return;
    const int lane = (int)(threadIdx.x & 63u);
    if (!((rec.mask >> lane) & 1ull)) return;
    const unsigned at = rec.first + (unsigned)__popcll(rec.mask & ((1ull << lane) - 1ull));
    if (at >= Q.cap) return;
    int c[3];
    (void)cell_of(Q, r, lane, c);
    float f[8];
    load_corners(Q, c, f);
    const unsigned classes = vrt_mesh::corner_classes(f);
    vrt_mesh::Vertex v;
    K::Probe P;
    float w[3], s[8], value = 0.0f;
    if (!candidate(Q, c, f, v, w, P, s, value)) return; /* (never: the count pass computed the same bits) */
    const int ja = vrt_mesh::material_corner(classes);
    const unsigned na = (unsigned)Q.A.N, nb = (unsigned)Q.B.N;
    const unsigned material_a = Q.material_a[((size_t)(c[0] + (ja & 1)) * na + (size_t)(c[2] + (ja >> 2))) * na + (size_t)(c[1] + ((ja >> 1) & 1))];
    int near[3];
    K::nearest_sample(Q.B, P, near);
    const unsigned material_b = Q.material_b[((size_t)near[0] * nb + (size_t)near[2]) * nb + (size_t)near[1]];
    const vrt_contact got = K::contact(Q.A, Q.B, c, w, v.n, material_a, P, s, value, material_b);
    cu4* out = reinterpret_cast<cu4*>(Q.out + at);
    out[0] = cu4{__float_as_uint(got.position[0]), __float_as_uint(got.position[1]), __float_as_uint(got.position[2]), __float_as_uint(got.distance)};
    out[1] = cu4{__float_as_uint(got.normal[0]), __float_as_uint(got.normal[1]), __float_as_uint(got.normal[2]), got.material_a};
    out[2] = cu4{__float_as_uint(got.normal_a[0]), __float_as_uint(got.normal_a[1]), __float_as_uint(got.normal_a[2]), got.material_b};
    out[3] = cu4{(unsigned)got.cell_a[0], (unsigned)got.cell_a[1], (unsigned)got.cell_a[2], 0u};
}

unsigned scan_blocks_of(unsigned n_runs) { return (n_runs + kScanThreads * kScanItems - 1) / (kScanThreads * kScanItems); }
size_t sums_bytes(unsigned n_runs) { return ((size_t)scan_blocks_of(n_runs) * sizeof(u64) + 255) / 256 * 256; }
Header* header_of(void* scratch) { return static_cast<Header*>(scratch); }
u64* sums_of(void* scratch) { return reinterpret_cast<u64*>(static_cast<char*>(scratch) + kHeaderBytes); }
Run* records_of(void* scratch, unsigned n_runs) { return reinterpret_cast<Run*>(static_cast<char*>(scratch) + kHeaderBytes + sums_bytes(n_runs)); }
/* the header, the scan's block sums and one 16-byte record per run */
size_t scratch_bytes(unsigned n_runs) { return kHeaderBytes + sums_bytes(n_runs) + (size_t)n_runs * sizeof(Run); }

/* An instance of the resident scene as the rule reads it: the placement as vrt_scene_set packed it, the slot as it is now. */
K::Side side_of(const vrt_ctx* ctx, int instance) {
    const DInstance& I = ctx->inst[instance];
    const HostVolume& h = ctx->vol[I.slot];
    K::Side s;
    memcpy(s.w2o, I.w2o, sizeof s.w2o);
    memcpy(s.o2w, I.o2w, sizeof s.o2w);
    memcpy(s.pos, I.pos, sizeof s.pos);
    s.smin = I.smin;
    K::grid(s, h.N, h.extent, h.format == VRT_FORMAT_TEXEL16, h.density_scale, h.step_max);
    return s;
}

/* Counts every run's contacts and turns the counts into the runs' first contact; the header gets the total and the smallest distance's
   key, the report (zeroed here) the candidates in the low half of `counts` and the contact cells' box. */
hipError_t launch_contacts_count(const DContacts& Q, void* scratch, hipStream_t stream) {
    hipError_t e = clear_report(Q.slots, stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(scratch, 0xff, kHeaderBytes, stream); /* min_key = kNoKey; the scan writes the total */
    if (e != hipSuccess) return e;
    const unsigned n_blocks = scan_blocks_of(Q.n_runs);
    hipLaunchKernelGGL(contacts_count_kernel, dim3((Q.n_runs + kRunsPerBlock - 1) / kRunsPerBlock), dim3(256), 0, stream, Q);
    hipLaunchKernelGGL(contacts_scan_reduce_kernel, dim3(n_blocks), dim3(kScanThreads), 0, stream, Q.runs, Q.n_runs, sums_of(scratch));
    hipLaunchKernelGGL(contacts_scan_sums_kernel, dim3(1), dim3(kScanThreads), 0, stream, sums_of(scratch), n_blocks, &header_of(scratch)->total);
    hipLaunchKernelGGL(contacts_scan_apply_kernel, dim3(n_blocks), dim3(kScanThreads), 0, stream, Q.runs, Q.n_runs, sums_of(scratch));
    return hipGetLastError();
}

hipError_t launch_contacts_emit(const DContacts& Q, hipStream_t stream) {
    hipLaunchKernelGGL(contacts_emit_kernel, dim3((Q.n_runs + kRunsPerBlock - 1) / kRunsPerBlock), dim3(256), 0, stream, Q);
    return hipGetLastError();
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_contact) == 64 && offsetof(vrt_contact, material_a) == 28 && offsetof(vrt_contact, normal_a) == 32 &&
                  offsetof(vrt_contact, cell_a) == 48 && sizeof(vrt_contacts_result) == 48,
              "contacts_emit_kernel writes four 16-B words per contact; vrt.h states the sizes");

extern "C" {

/* vrt_query_contacts, on device 0: the host clips A's cells to where B's box can reach (contacts_core.h's cell_box), the runs of that
 * box are counted and scanned (launch_contacts_count), the host reads the total, the smallest distance's key and the report, checks the
 * caller's capacity and sizes the staged records, the runs write them (launch_contacts_emit) and they are copied out.  Both slots are
 * only read. */
int vrt_query_contacts(vrt_ctx* ctx, int instance_a, int instance_b, float margin, vrt_contact* contacts, size_t capacity, vrt_contacts_result* result) {
    if (!ctx || !result || !std::isfinite(margin) || margin < 0.0f) return VRT_ERR_INVALID;
    if ((!contacts && capacity > 0) || instance_a == instance_b) return VRT_ERR_INVALID;
    if (!ctx->have_scene) return VRT_ERR_NOT_READY;
    const int n_inst = ctx->scene.n_instances;
    if (instance_a < 0 || instance_a >= n_inst || instance_b < 0 || instance_b >= n_inst) return VRT_ERR_INVALID;
    const int slot_a = ctx->scene.instances[instance_a].volume_slot, slot_b = ctx->scene.instances[instance_b].volume_slot;
    if (!ctx->vol[slot_a].used || !ctx->vol[slot_b].used) return VRT_ERR_SLOT; /* (freed since the scene was set) */
    DeviceState& D = ctx->dev[0];
    {
        DFrame F; /* a scene set that was deferred while frames were in flight is applied, as for vrt_query_points */
        const int rc = query_scene(ctx, D.stream, F);
        if (rc != VRT_OK) return rc;
    }
    int rc = quiesce(ctx);
    if (rc != VRT_OK) return rc;
    DContacts Q;
    memset(&Q, 0, sizeof Q); /* (the whole struct travels as the kernarg) */
    Q.A = side_of(ctx, instance_a);
    Q.B = side_of(ctx, instance_b);
    const int N = Q.A.N;
    vrt_contacts_result got = {{N, N, N}, {-1, -1, -1}, 0, 0, INFINITY, 0};
    int lo[3], hi[3];
    if (K::cell_box(Q.A, Q.B, lo, hi)) {
        for (int a = 0; a < 3; a++) Q.lo[a] = lo[a], Q.n[a] = hi[a] - lo[a] + 1;
        Q.runs_y = (Q.n[1] + 63) / 64;
        Q.n_runs = (unsigned)Q.n[0] * (unsigned)Q.n[2] * (unsigned)Q.runs_y;
        Q.margin = margin;
        Q.dense_a = D.vol[slot_a].dense, Q.material_a = D.vol[slot_a].material;
        Q.dense_b = D.vol[slot_b].dense, Q.material_b = D.vol[slot_b].material;
        HIP_TRY(hipSetDevice(D.ordinal));
        rc = ensure_buffer(D.buf[kBufMeshScratch], scratch_bytes(Q.n_runs));
        if (rc != VRT_OK) return rc;
        void* scratch = D.buf[kBufMeshScratch].p;
        Q.runs = records_of(scratch, Q.n_runs);
        Q.header = header_of(scratch);
        Q.slots = D.d_brush;
        HIP_TRY(launch_contacts_count(Q, scratch, D.stream));
        Header head;
        Written cells; /* the contact cells' box, the candidates in `low` */
        HIP_TRY(hipMemcpyAsync(&head, Q.header, sizeof head, hipMemcpyDeviceToHost, D.stream));
        rc = read_report(D, N, cells); /* the header arrives in the same synchronisation */
        if (rc != VRT_OK) return rc;
        got.contacts = head.total;
        got.candidates = cells.low;
        got.min_distance = K::key_distance(head.min_key);
        for (int a = 0; a < 3; a++) got.lo[a] = cells.lo[a], got.hi[a] = cells.hi[a];
    }
    *result = got;
    if (!contacts) return VRT_OK;
    if (capacity < got.contacts) return VRT_ERR_INVALID;
    if (got.contacts == 0) return VRT_OK;
    const size_t bytes = (size_t)got.contacts * sizeof(vrt_contact);
    rc = ensure_buffer(D.buf[kBufMeshOut], bytes);
    if (rc != VRT_OK) return rc;
    Q.out = static_cast<vrt_contact*>(D.buf[kBufMeshOut].p);
    Q.cap = (unsigned)got.contacts;
    HIP_TRY(launch_contacts_emit(Q, D.stream));
    HIP_TRY(hipMemcpyAsync(contacts, Q.out, bytes, hipMemcpyDeviceToHost, D.stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    return VRT_OK;
}

}  // extern "C"
