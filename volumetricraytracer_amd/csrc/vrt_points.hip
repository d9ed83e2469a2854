/* vrt_points.hip — vrt_query_points (include/vrt.h), kernel to driver: how far a world point is from the nearest surface of the
 * resident scene, in which direction, and (iterations > 0) where the nearest surface point is.
 *
 * One lane per point, 256-lane workgroups, no LDS.  The loop over the scene's instances is wave-uniform, so an instance's record and its
 * volume's come through scalar loads; the lanes differ only in whether their point lies in the instance's box, where they sample the
 * dense grid trilinearly, or outside it, where the distance to the box is the bound.  The dense grid holds N^3 floats on either format
 * (the integer field on VRT_FORMAT_TEXEL16), so one code path serves both and nothing else of a slot is read but its material ids.
 * The eight taps of a lane share nothing with its neighbours': few registers, and occupancy hides the gather, as in vrt_stamp.hip.  The
 * taps are four y-adjacent pairs (grid_device.h's load_taps).  The rule's steps are csrc/points_core.h's, which vrt_query_contacts
 * shares; this file feeds them from the scene's records and keeps the minimum over the instances.  A projection re-enters the
 * evaluation, which is why its loop is not unrolled.  The 16-B point is one load, the 64-B record four 16-B stores. */
#include <hip/hip_runtime.h>

#include <string.h>

#include <cmath>

#include "grid_device.h"
#include "points_core.h"
#include "vrt_context.h"

namespace vrt {

namespace {

constexpr int kPointThreads = 256;
typedef float pf4 __attribute__((ext_vector_type(4)));
typedef unsigned pu4 __attribute__((ext_vector_type(4)));

/* The kernarg of a launch.  vols / inst / n_inst: the scene as build_frame fills a ray query's; material: the slots' N^3 material grids,
   as DQuery::material; density_scale: the caller's per slot, without the 0.01 that DVolume::density_scale folds in on VRT_FORMAT_TEXEL16
   (the rule decodes every corner sample first). */
struct DPoints {
    const DVolume* vols;
    const DInstance* inst;
    const void* points; /* n vrt_point records (16 B) */
    void* results;      /* n vrt_point_result records (64 B) */
    int32_t n, n_inst;
    int32_t iterations;
    float tolerance;
    const uint8_t* material[VRT_MAX_VOLUMES];
    float density_scale[VRT_MAX_VOLUMES];
};

namespace P = vrt_points;

/* What a lane keeps of the best instance so far while it walks the scene. */
struct Best {
    float value;        /* the minimum; +inf with instance -1 */
    int instance;
    bool sampled;
    float h[3];         /* w2o^T G of a sampled minimum */
    int v[3];           /* its nearest grid sample */
    const uint8_t* mat; /* that sample's material id, or null */
};

/* E(p) of the rule in vrt.h, steps 1-5 and the h of step 6. */
__device__ __forceinline__ void evaluate(const DPoints& Q, float px, float py, float pz, Best& B) {
    const float p[3] = {px, py, pz};
    B.value = __builtin_inff();
    B.instance = -1;
    B.sampled = false;
    B.h[0] = B.h[1] = B.h[2] = 0.0f;
    B.v[0] = B.v[1] = B.v[2] = -1;
    B.mat = nullptr;
    if (!P::finite(p)) return;
    for (int k = 0; k < Q.n_inst; k++) {
        const DInstance* __restrict__ I = Q.inst + k;
        const int slot = I->slot;
        const DVolume* __restrict__ V = Q.vols + slot;
        const float ext = V->extent, smin = I->smin;
        float q[3], e[3], value;
        P::object_point(I->w2o, I->pos, p, q);
        if (P::in_box(q, ext, e)) {
            const int N = V->N;
            const bool t16 = V->format == VRT_FORMAT_TEXEL16; /* read here, beside N: read at the call below it costs two VGPRs */
            float g[3], f[3], s[8];
            int c[3];
            P::cell_and_fractions(q, ext, V->inv_cell, N, g, c, f);
            load_taps(V->dense, N, c, t16, s);
            /* step_max: +inf for a slot whose step_max is not positive (fill_dvolume) */
            if (!P::value_at(s, f, Q.density_scale[slot], V->step_max, smin, value)) continue; /* contributes nothing */
            if (!(B.instance < 0 || value < B.value)) continue;
            float G[3];
            P::gradient_at(s, f, G);
            P::transposed_times(I->w2o, G, B.h);
            P::nearest_sample(g, N, B.v);
            const uint8_t* mat = Q.material[slot];
            const unsigned n = (unsigned)N;
            B.mat = mat != nullptr ? mat + (((unsigned)B.v[0] * n + (unsigned)B.v[2]) * n + (unsigned)B.v[1]) : nullptr;
            B.sampled = true;
        } else {
            value = P::box_bound(e, smin);
            if (!(B.instance < 0 || value < B.value)) continue;
            B.sampled = false;
        }
        B.value = value;
        B.instance = k;
    }
}

__global__ __launch_bounds__(kPointThreads) void points_kernel(const DPoints Q) {
    const unsigned i = blockIdx.x * (unsigned)kPointThreads + threadIdx.x;
    if (i >= (unsigned)Q.n) return;
    const pf4 rec = reinterpret_cast<const pf4*>(Q.points)[i];
    float px = rec.x, py = rec.y, pz = rec.z;
    unsigned moves = 0u;
    Best B;
    float n[3];
#pragma nounroll
    for (;;) {
        evaluate(Q, px, py, pz, B);
        n[0] = n[1] = n[2] = 0.0f;
        if (B.sampled) P::normalised(B.h, n);
        if (moves >= (unsigned)Q.iterations || !B.sampled || (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) || fabsf(B.value) <= Q.tolerance) break;
        px = px - (n[0] * B.value);
        py = py - (n[1] * B.value);
        pz = pz - (n[2] * B.value);
        moves++;
    }
    unsigned material = 0u;
    if (B.sampled && B.mat != nullptr) material = *B.mat;
    if (!B.sampled) B.v[0] = B.v[1] = B.v[2] = -1;
    pu4* out = reinterpret_cast<pu4*>(Q.results) + 4 * (size_t)i;
    out[0] = pu4{__float_as_uint(B.value), __float_as_uint(n[0]), __float_as_uint(n[1]), __float_as_uint(n[2])};
    out[1] = pu4{(unsigned)B.instance, (unsigned)B.v[0], (unsigned)B.v[1], (unsigned)B.v[2]};
    out[2] = pu4{material, B.sampled ? (unsigned)VRT_POINT_SAMPLED : 0u, moves, __float_as_uint(px)};
    out[3] = pu4{__float_as_uint(py), __float_as_uint(pz), 0u, 0u};
}

/* What vrt_query_points and vrt_query_points_host refuse, checked before anything is enqueued. */
int check_points(const vrt_ctx* ctx, int iterations, float tolerance, int n, const void* points, const void* results) {
    if (!ctx || n < 0 || (n > 0 && (!points || !results))) return VRT_ERR_INVALID;
    if (iterations < 0 || iterations > VRT_MAX_PROJECT_ITERATIONS || !std::isfinite(tolerance) || tolerance < 0.0f) return VRT_ERR_INVALID;
    if (!ctx->have_scene) return VRT_ERR_NOT_READY;
    return VRT_OK;
}

/* One launch of n points on the first device.  Touches none of the render's bookkeeping; allocates nothing. */
int enqueue_points(vrt_ctx* ctx, int iterations, float tolerance, int n, const void* points, void* results, hipStream_t stream) {
    DFrame F;
    const int rc = query_scene(ctx, stream, F);
    if (rc != VRT_OK) return rc;
    const DeviceState& D = ctx->dev[0];
    DPoints Q;
    memset(&Q, 0, sizeof Q); /* (the whole struct travels as the kernarg) */
    Q.vols = F.vols;
    Q.inst = F.inst;
    Q.n_inst = F.n_inst;
    Q.points = points;
    Q.results = results;
    Q.n = n;
    Q.iterations = iterations;
    Q.tolerance = tolerance;
    for (int s = 0; s < VRT_MAX_VOLUMES; s++) {
        Q.material[s] = D.vol[s].material;
        Q.density_scale[s] = ctx->vol[s].density_scale;
    }
    const dim3 g(((unsigned)n + (unsigned)kPointThreads - 1u) / (unsigned)kPointThreads), t(kPointThreads);
    hipLaunchKernelGGL(points_kernel, g, t, 0, stream, Q);
    HIP_TRY(hipGetLastError());
    return VRT_OK;
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_point) == 16 && sizeof(vrt_point_result) == 64 && offsetof(vrt_point_result, position) == 44,
              "points_kernel reads one and writes four 16-B words per point");

extern "C" {

int vrt_query_points(vrt_ctx* ctx, int iterations, float tolerance, int n, const vrt_point* device_points, vrt_point_result* device_results,
                     void* hip_stream) {
    const int rc = check_points(ctx, iterations, tolerance, n, device_points, device_results);
    if (rc != VRT_OK || n == 0) return rc;
    return enqueue_points(ctx, iterations, tolerance, n, device_points, device_results, static_cast<hipStream_t>(hip_stream));
}

int vrt_query_points_host(vrt_ctx* ctx, int iterations, float tolerance, int n, const vrt_point* points, vrt_point_result* results) {
    int rc = check_points(ctx, iterations, tolerance, n, points, results);
    if (rc != VRT_OK || n == 0) return rc;
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    const size_t in_bytes = sizeof(vrt_point) * (size_t)n, out_bytes = sizeof(vrt_point_result) * (size_t)n;
    rc = ensure_buffer(D.buf[kBufQuery], in_bytes + out_bytes);
    if (rc != VRT_OK) return rc;
    char* base = static_cast<char*>(D.buf[kBufQuery].p);
    HIP_TRY(hipMemcpyAsync(base, points, in_bytes, hipMemcpyHostToDevice, D.stream));
    rc = enqueue_points(ctx, iterations, tolerance, n, base, base + in_bytes, D.stream);
    if (rc != VRT_OK) {
        (void)hipStreamSynchronize(D.stream);
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(results, base + in_bytes, out_bytes, hipMemcpyDeviceToHost, D.stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    return VRT_OK;
}

}  // extern "C"
