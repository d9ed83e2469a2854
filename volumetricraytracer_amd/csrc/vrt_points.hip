/* vrt_points.hip — vrt_query_points (include/vrt.h), kernel to driver: how far a world point is from the nearest surface of the
 * resident scene, in which direction, and (iterations > 0) where the nearest surface point is.
 *
 * One lane per point, 256-lane workgroups, no LDS.  The loop over the scene's instances is wave-uniform, so an instance's record and its
 * volume's come through scalar loads; the lanes differ only in whether their point lies in the instance's box, where they sample the
 * dense grid trilinearly, or outside it, where the distance to the box is the bound.  The dense grid holds N^3 floats on either format
 * (the integer field on VRT_FORMAT_TEXEL16), so one code path serves both and nothing else of a slot is read but its material ids.
 * The eight taps of a lane share nothing with its neighbours': few registers, and occupancy hides the gather, as in vrt_stamp.hip.  The
 * taps are four y-adjacent pairs, written as adjacent loads for the compiler to merge into 8-byte ones (the fp32 bricks' fetch of the
 * march does the same; tools/microbench/gather16.hip checked such loads at 4-byte alignment).  A projection re-enters the evaluation,
 * which is why its loop is not unrolled.  The 16-B point is one load, the 64-B record four 16-B stores. */
#include <hip/hip_runtime.h>

#include <string.h>

#include <cmath>

#include "grid_core.h"
#include "vrt_context.h"

namespace vrt {

namespace {

constexpr int kPointThreads = 256;
typedef float pf4 __attribute__((ext_vector_type(4)));
typedef unsigned pu4 __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) * pgfloat_p;

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

__device__ __forceinline__ float lerp(float s0, float s1, float f) { return (s0 * (1.0f - f)) + (s1 * f); }
__device__ __forceinline__ float dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

/* What a lane keeps of the best instance so far while it walks the scene. */
struct Best {
    float value;        /* the minimum; +inf with instance -1 */
    int instance;
    bool sampled;
    float hx, hy, hz;   /* w2o^T G of a sampled minimum */
    int vx, vy, vz;     /* its nearest grid sample */
    const uint8_t* mat; /* that sample's material id, or null */
};

/* E(p) of the rule in vrt.h, steps 1-5 and the h of step 6. */
__device__ __forceinline__ void evaluate(const DPoints& Q, float px, float py, float pz, Best& B) {
    B.value = __builtin_inff();
    B.instance = -1;
    B.sampled = false;
    B.hx = B.hy = B.hz = 0.0f;
    B.vx = B.vy = B.vz = -1;
    B.mat = nullptr;
    if (!(__builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz))) return;
    for (int k = 0; k < Q.n_inst; k++) {
        const DInstance* __restrict__ I = Q.inst + k;
        const int slot = I->slot;
        const DVolume* __restrict__ V = Q.vols + slot;
        const float* m = I->w2o;
        const float rx = px - I->pos[0], ry = py - I->pos[1], rz = pz - I->pos[2];
        const float qx = dot(m[0], m[1], m[2], rx, ry, rz), qy = dot(m[3], m[4], m[5], rx, ry, rz), qz = dot(m[6], m[7], m[8], rx, ry, rz);
        const float ext = V->extent, smin = I->smin;
        const float ex = fabsf(qx) - ext, ey = fabsf(qy) - ext, ez = fabsf(qz) - ext;
        float value;
        if (ex <= 0.0f && ey <= 0.0f && ez <= 0.0f) {
            const int N = V->N;
            const float ic = V->inv_cell;
            const float gx = (qx + ext) * ic, gy = (qy + ext) * ic, gz = (qz + ext) * ic;
            const int cx = min(max((int)floorf(gx), 0), N - 2), cy = min(max((int)floorf(gy), 0), N - 2), cz = min(max((int)floorf(gz), 0), N - 2);
            const float fx = gx - (float)cx, fy = gy - (float)cy, fz = gz - (float)cz;
            /* [x][z][y], 0 <= c <= N - 2 on every axis: all eight taps lie inside the grid; N <= 513, so a byte offset fits 32 bits */
            const unsigned n = (unsigned)N;
            const unsigned at = ((unsigned)cx * n + (unsigned)cz) * n + (unsigned)cy;
            const pgfloat_p b00 = (pgfloat_p)(V->dense) + at; /* x, z */
            const pgfloat_p b01 = b00 + n, b10 = b00 + n * n, b11 = b10 + n;
            const bool t16 = V->format == VRT_FORMAT_TEXEL16;
            /* s<dx><dy><dz> */
            const float s000 = vrt_grid::decode(b00[0], t16), s010 = vrt_grid::decode(b00[1], t16);
            const float s001 = vrt_grid::decode(b01[0], t16), s011 = vrt_grid::decode(b01[1], t16);
            const float s100 = vrt_grid::decode(b10[0], t16), s110 = vrt_grid::decode(b10[1], t16);
            const float s101 = vrt_grid::decode(b11[0], t16), s111 = vrt_grid::decode(b11[1], t16);
            const float t = lerp(lerp(lerp(s000, s100, fx), lerp(s010, s110, fx), fy), lerp(lerp(s001, s101, fx), lerp(s011, s111, fx), fy), fz);
            if (t != t) continue; /* contributes nothing */
            float d = t * Q.density_scale[slot];
            const float sm = V->step_max; /* +inf for a slot whose step_max is not positive (fill_dvolume) */
            if (sm < __builtin_inff() && sm > 0.0f) d = fminf(d, sm);
            value = d * smin;
            if (!(B.instance < 0 || value < B.value)) continue;
            const float Gx = lerp(lerp(s100 - s000, s110 - s010, fy), lerp(s101 - s001, s111 - s011, fy), fz);
            const float Gy = lerp(lerp(s010 - s000, s110 - s100, fx), lerp(s011 - s001, s111 - s101, fx), fz);
            const float Gz = lerp(lerp(s001 - s000, s101 - s100, fx), lerp(s011 - s010, s111 - s110, fx), fy);
            B.hx = (m[0] * Gx + m[3] * Gy) + m[6] * Gz;
            B.hy = (m[1] * Gx + m[4] * Gy) + m[7] * Gz;
            B.hz = (m[2] * Gx + m[5] * Gy) + m[8] * Gz;
            /* the nearest grid sample, as vrt_hit::voxel */
            const float nmax = (float)(N - 1);
            B.vx = (int)__builtin_amdgcn_fmed3f(floorf(gx + 0.5f), 0.0f, nmax);
            B.vy = (int)__builtin_amdgcn_fmed3f(floorf(gy + 0.5f), 0.0f, nmax);
            B.vz = (int)__builtin_amdgcn_fmed3f(floorf(gz + 0.5f), 0.0f, nmax);
            const uint8_t* mat = Q.material[slot];
            B.mat = mat != nullptr ? mat + (((unsigned)B.vx * n + (unsigned)B.vz) * n + (unsigned)B.vy) : nullptr;
            B.sampled = true;
        } else {
            const float mx = fmaxf(ex, 0.0f), my = fmaxf(ey, 0.0f), mz = fmaxf(ez, 0.0f);
            value = sqrtf(dot(mx, my, mz, mx, my, mz)) * smin;
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
    float nx, ny, nz;
#pragma nounroll
    for (;;) {
        evaluate(Q, px, py, pz, B);
        nx = ny = nz = 0.0f;
        if (B.sampled) {
            const float H = dot(B.hx, B.hy, B.hz, B.hx, B.hy, B.hz);
            if (H != 0.0f && __builtin_isfinite(H)) {
                const float len = sqrtf(H);
                nx = B.hx / len;
                ny = B.hy / len;
                nz = B.hz / len;
            }
        }
        if (moves >= (unsigned)Q.iterations || !B.sampled || (nx == 0.0f && ny == 0.0f && nz == 0.0f) || fabsf(B.value) <= Q.tolerance) break;
        px = px - (nx * B.value);
        py = py - (ny * B.value);
        pz = pz - (nz * B.value);
        moves++;
    }
    unsigned material = 0u;
    if (B.sampled && B.mat != nullptr) material = *B.mat;
    if (!B.sampled) B.vx = B.vy = B.vz = -1;
    pu4* out = reinterpret_cast<pu4*>(Q.results) + 4 * (size_t)i;
    out[0] = pu4{__float_as_uint(B.value), __float_as_uint(nx), __float_as_uint(ny), __float_as_uint(nz)};
    out[1] = pu4{(unsigned)B.instance, (unsigned)B.vx, (unsigned)B.vy, (unsigned)B.vz};
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
