/* vrt_contacts.hip — vrt_query_contacts (include/vrt.h), kernels to driver: the surface points of instance A that lie in or near
 * instance B, as compact records in the order of A's cells.  The rule is csrc/contacts_core.h over csrc/mesh_core.h and
 * csrc/points_core.h; the walk over runs of 64 cells of the clipped cell box of A, the runs' records, their scan and the loads of
 * corners and taps are csrc/grid_device.h's, which vrt_mesh.hip shares.
 *   count   every lane loads its cell's eight corners of A (y fastest: coalesced rows); the few active lanes make the vertex, take it to
 *           the world and into B, and fetch B's eight taps there — load_taps, as vrt_points.hip does, on the sparse active
 *           lanes as they are (DESIGN §2 has why) — and the contact test goes through __ballot into the run's 16-byte record.  The
 *           wave's candidates and its contacts' cell box leave through the edit report, the smallest distance through one atomicMin on
 *           an order-preserving key: integers all, which no order of waves can change.
 *   scan    launch_run_scan: the counts become the runs' first contact; the total is the low half of the scratch's first word.
 *   emit    a run with a non-empty mask recomputes its contact lanes with the same inline function — the same bits — and writes each
 *           record as four 16-byte stores at first + popcount(mask below the lane).  No N^3 index volume, no atomics on the order.
 * A's and B's descriptors are wave-uniform and travel in the kernarg: they come through scalar loads. */
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <cmath>

#include "contacts_core.h"
#include "grid_device.h"
#include "vrt_context.h"

namespace vrt {

namespace {

namespace K = vrt_contacts;

typedef unsigned cu4 __attribute__((ext_vector_type(4)));

/* The head of the scratch, on top of grid_device.h's layout. */
struct Header {
    u64 total;        /* the scan's totals word: contacts in the low half, the high half 0 */
    unsigned min_key; /* contacts_core.h's distance_key of the smallest distance; kNoKey: none */
};
static_assert(offsetof(Header, total) == 0 && sizeof(Header) <= kRunHeaderBytes, "the scan writes its totals to the scratch's first word");

/* The kernarg of count and emit. */
struct DContacts {
    K::Side A, B;
    const float* dense_a;
    const uint8_t* material_a;
    const float* dense_b;
    const uint8_t* material_b;
    RunGrid G; /* the clipped cell box of A */
    unsigned n_runs;
    float margin;
    Run* runs;
    Header* header;
    DBrushSlot* slots;
    vrt_contact* out; /* emit */
    unsigned cap;
};

/* What count and emit both compute of an ACTIVE cell c of A with the corner values f: its vertex, the world point, where that falls
   in B, B's decoded taps and value.  False: no candidate (nothing but v and w is set then). */
__device__ __forceinline__ bool candidate(const DContacts& Q, const int c[3], const float f[8], vrt_mesh::Vertex& v, float w[3], K::Probe& P,
                                          float s[8], float& value) {
    v = vrt_mesh::cell_vertex(c, f);
    K::world_point(Q.A, v.p, w);
    if (!K::probe(Q.B, w, P)) return false;
    load_taps(Q.dense_b, Q.B.N, P.c, Q.B.texel16 != 0, s);
    return K::value_of(Q.B, P, s, value);
}

__global__ __launch_bounds__(256) void contacts_count_kernel(const DContacts Q) {
    const unsigned r = blockIdx.x * kRunsPerBlock + (threadIdx.x >> 6);
    if (r >= Q.n_runs) return; /* the whole wave */
    const int lane = (int)(threadIdx.x & 63u);
    int c[3];
    bool cand = false, hit = false;
    float value = 0.0f;
    if (cell_of(Q.G, r, lane, c)) {
        float f[8];
        load_corners(Q.dense_a, Q.A.N, c, 0.0f, Q.A.texel16 != 0, f);
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
    rec.mask = mask, rec.count[0] = (unsigned)__popcll(mask), rec.count[1] = 0u;
    Q.runs[r] = rec;
    if (cands == 0ull) return;
    EditReport report;
    report.n_low = report.n_low_only = (unsigned)__popcll(cands); /* the candidates: the low half of `counts` */
    if (mask != 0ull) {
        bound_run(report, Q.A.N, c, mask);
        atomicMin(&Q.header->min_key, key);
    }
    report.write(Q.slots, r);
}

__global__ __launch_bounds__(256) void contacts_emit_kernel(const DContacts Q) {
    const unsigned r = blockIdx.x * kRunsPerBlock + (threadIdx.x >> 6);
    if (r >= Q.n_runs) return; /* the whole wave */
    const Run rec = Q.runs[r];
    if (rec.mask == 0ull) return;
    const int lane = (int)(threadIdx.x & 63u);
    if (!((rec.mask >> lane) & 1ull)) return;
    const unsigned at = number_in(rec, lane);
    if (at >= Q.cap) return;
    int c[3];
    (void)cell_of(Q.G, r, lane, c);
    float f[8];
    load_corners(Q.dense_a, Q.A.N, c, 0.0f, Q.A.texel16 != 0, f);
    const unsigned classes = vrt_mesh::corner_classes(f);
    vrt_mesh::Vertex v;
    K::Probe P;
    float w[3], s[8], value = 0.0f;
    if (!candidate(Q, c, f, v, w, P, s, value)) return; /* (never: the count pass computed the same bits) */
    const int ja = vrt_mesh::material_corner(classes);
    const unsigned na = (unsigned)Q.A.N, nb = (unsigned)Q.B.N;
    const unsigned material_a = Q.material_a[((size_t)(c[0] + (ja & 1)) * na + (size_t)(c[2] + (ja >> 2))) * na + (size_t)(c[1] + ((ja >> 1) & 1))];
    int near[3];
    vrt_points::nearest_sample(P.g, Q.B.N, near);
    const unsigned material_b = Q.material_b[((size_t)near[0] * nb + (size_t)near[2]) * nb + (size_t)near[1]];
    const vrt_contact got = K::contact(Q.A, Q.B, c, w, v.n, material_a, P, s, value, material_b);
    cu4* out = reinterpret_cast<cu4*>(Q.out + at);
    out[0] = cu4{__float_as_uint(got.position[0]), __float_as_uint(got.position[1]), __float_as_uint(got.position[2]), __float_as_uint(got.distance)};
    out[1] = cu4{__float_as_uint(got.normal[0]), __float_as_uint(got.normal[1]), __float_as_uint(got.normal[2]), got.material_a};
    out[2] = cu4{__float_as_uint(got.normal_a[0]), __float_as_uint(got.normal_a[1]), __float_as_uint(got.normal_a[2]), got.material_b};
    out[3] = cu4{(unsigned)got.cell_a[0], (unsigned)got.cell_a[1], (unsigned)got.cell_a[2], 0u};
}

Header* header_of(void* scratch) { return static_cast<Header*>(scratch); }

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
    e = hipMemsetAsync(scratch, 0xff, kRunHeaderBytes, stream); /* min_key = kNoKey; the scan writes the total */
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(contacts_count_kernel, dim3((Q.n_runs + kRunsPerBlock - 1) / kRunsPerBlock), dim3(256), 0, stream, Q);
    launch_run_scan(Q.runs, Q.n_runs, scratch, stream);
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
        Q.G = run_grid(N, lo, hi);
        Q.n_runs = runs_of(Q.G);
        Q.margin = margin;
        Q.dense_a = D.vol[slot_a].dense, Q.material_a = D.vol[slot_a].material;
        Q.dense_b = D.vol[slot_b].dense, Q.material_b = D.vol[slot_b].material;
        HIP_TRY(hipSetDevice(D.ordinal));
        rc = ensure_buffer(D.buf[kBufMeshScratch], run_scratch_bytes(Q.n_runs));
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
