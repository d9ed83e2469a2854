/* vrt_sweeps.hip — vrt_query_sweeps (include/vrt.h), kernel to driver: where a sphere of radius r, its centre moved along a line, first
 * touches the resident scene.
 *
 * One lane per record, 256-lane workgroups, no LDS, in the shape of vrt_points.hip: the loop over the scene's instances is wave-uniform,
 * so an instance's record and its volume's come through scalar loads, and the eight taps of a lane are four y-adjacent pairs
 * (grid_device.h's load_taps) that occupancy hides.  A record's candidates (the rule's step 2) are a 64-bit mask per lane, built once;
 * an evaluation skips an instance outright when no active lane of the wave holds it.  The step loop is not unrolled and carries
 * (c, k, sampled, t, steps) only: the gradient, the nearest sample and the material of a HIT come from evaluating the winning instance
 * once more at the final centre, after the loop — the same functions on the same values, hence the same bits.  The rule's own steps
 * are csrc/sweep_core.h's, the per-instance ones csrc/points_core.h's.  The lanes of a wave differ in how many steps they take, and the
 * wave lives as long as its slowest lane (profiles/sweeps.txt has what that costs).  The 32-B record is two 16-B loads, the 64-B
 * record four 16-B stores. */
#include <hip/hip_runtime.h>

#include <string.h>

#include <cmath>

#include "grid_device.h"
#include "sweep_core.h"
#include "vrt_context.h"

namespace vrt {

namespace {

constexpr int kSweepThreads = 256;
typedef float sf4 __attribute__((ext_vector_type(4)));
typedef unsigned su4 __attribute__((ext_vector_type(4)));

/* The kernarg of a launch.  vols / inst / n_inst, material and density_scale: as vrt_points.hip's DPoints.  reach: Rb of the rule's
   step 2 per instance, computed on the host from the resident scene's scales (DInstance has no word left for it). */
struct DSweeps {
    const DVolume* vols;
    const DInstance* inst;
    const void* sweeps; /* n vrt_sweep records (32 B) */
    void* hits;         /* n vrt_sweep_hit records (64 B) */
    int32_t n, n_inst;
    int32_t max_steps;
    float tolerance, step_min;
    const uint8_t* material[VRT_MAX_VOLUMES];
    float density_scale[VRT_MAX_VOLUMES];
    float reach[VRT_MAX_INSTANCES];
};

namespace P = vrt_points;
namespace S = vrt_sweeps;

enum { kNothing = 0, kBound = 1, kSampled = 2 };

/* What the record of a HIT takes from the points rule's step 6. */
struct Fields {
    float h[3];
    int v[3];
    const uint8_t* mat;
};

/* The points rule's steps 1 to 4 for instance k alone at p: its value, and whether it is a sample, a box bound or nothing.  kFields:
   step 6's h, nearest sample and material address of a sample as well. */
template <bool kFields>
__device__ __forceinline__ int instance_at(const DSweeps& Q, int k, const float p[3], float& value, Fields& F) {
    const DInstance* __restrict__ I = Q.inst + k;
    const int slot = I->slot;
    const DVolume* __restrict__ V = Q.vols + slot;
    const float ext = V->extent, smin = I->smin;
    float q[3], e[3];
    P::object_point(I->w2o, I->pos, p, q);
    if (!P::in_box(q, ext, e)) {
        value = P::box_bound(e, smin);
        return kBound;
    }
    const int N = V->N;
    const bool t16 = V->format == VRT_FORMAT_TEXEL16;
    float g[3], f[3], s[8];
    int c[3];
    P::cell_and_fractions(q, ext, V->inv_cell, N, g, c, f);
    load_taps(V->dense, N, c, t16, s);
    if (!P::value_at(s, f, Q.density_scale[slot], V->step_max, smin, value)) return kNothing;
    if (kFields) {
        float G[3];
        P::gradient_at(s, f, G);
        P::transposed_times(I->w2o, G, F.h);
        P::nearest_sample(g, N, F.v);
        const uint8_t* mat = Q.material[slot];
        const unsigned n = (unsigned)N;
        F.mat = mat != nullptr ? mat + (((unsigned)F.v[0] * n + (unsigned)F.v[2]) * n + (unsigned)F.v[1]) : nullptr;
    }
    return kSampled;
}

/* Whether any active lane of the wave says yes. */
__device__ __forceinline__ bool wave_any(bool yes) { return __builtin_amdgcn_ballot_w64(yes) != 0ull; }

__device__ __forceinline__ void store_record(void* hits, unsigned i, const uint32_t w[16]) {
    su4* out = reinterpret_cast<su4*>(hits) + 4 * (size_t)i;
    out[0] = su4{w[0], w[1], w[2], w[3]};
    out[1] = su4{w[4], w[5], w[6], w[7]};
    out[2] = su4{w[8], w[9], w[10], w[11]};
    out[3] = su4{w[12], w[13], w[14], w[15]};
}

__global__ __launch_bounds__(kSweepThreads) void sweeps_kernel(const DSweeps Q) {
    const unsigned i = blockIdx.x * (unsigned)kSweepThreads + threadIdx.x;
    if (i >= (unsigned)Q.n) return;
    const sf4 ra = reinterpret_cast<const sf4*>(Q.sweeps)[2 * (size_t)i], rb = reinterpret_cast<const sf4*>(Q.sweeps)[2 * (size_t)i + 1];
    const float o[3] = {ra.x, ra.y, ra.z}, d[3] = {rb.x, rb.y, rb.z};
    const float t_max = ra.w, radius = rb.w;
    float L, u[3] = {0.0f, 0.0f, 0.0f};
    const bool bad = S::bad_record(o, d, t_max, radius, L);
    unsigned long long cand = 0ull;
    if (!bad) {
        S::direction(d, L, u);
        for (int k = 0; k < Q.n_inst; k++)
            if (S::candidate(Q.inst[k].pos, o, u, t_max, Q.reach[k], radius)) cand |= 1ull << k;
    }
    float t = 0.0f, c = 0.0f, p[3] = {o[0], o[1], o[2]};
    unsigned steps = 0u, flags = 0u;
    int best = -1;
    if (!bad) {
#pragma nounroll
        for (;;) {
            S::point_at(o, u, t, p);
            if (t > t_max) break;
            if (steps == (unsigned)Q.max_steps) {
                flags = S::kExhausted;
                break;
            }
            steps++;
            bool sampled = false;
            best = -1;
            if (P::finite(p)) {
                for (int k = 0; k < Q.n_inst; k++) {
                    const bool mine = ((cand >> k) & 1ull) != 0ull;
                    if (!wave_any(mine)) continue; /* no active lane holds instance k */
                    if (!mine) continue;
                    float value;
                    Fields unused;
                    const int kind = instance_at<false>(Q, k, p, value, unused);
                    if (kind == kNothing) continue;
                    const float ck = S::clearance(value, kind == kSampled, radius);
                    if (!S::takes(ck, best, c)) continue;
                    c = ck, best = k, sampled = kind == kSampled;
                }
            }
            if (best < 0) break;
            if (S::touches(sampled, c, Q.tolerance)) {
                flags = S::kHit;
                break;
            }
            t = S::advance(t, c, Q.step_min);
        }
    }
    uint32_t w[16];
    S::no_hit_record(flags, t, steps, p, w);
    if (flags & S::kHit) {
        /* the winning instance once more, for what the loop does not carry; the loop over k stays wave-uniform */
        for (int k = 0; k < Q.n_inst; k++) {
            if (!wave_any(k == best)) continue;
            if (k != best) continue;
            /* (inside this branch the compiler knows k == best and would index the records by the lane's `best`, with vector loads) */
            const int ku = __builtin_amdgcn_readfirstlane(k);
            float value;
            Fields F;
            (void)instance_at<true>(Q, ku, p, value, F);
            const unsigned material = F.mat != nullptr ? *F.mat : 0u;
            S::hit_record(t, steps, p, ku, value, F.h, F.v, material, w);
        }
    }
    store_record(Q.hits, i, w);
}

/* What vrt_query_sweeps and vrt_query_sweeps_host refuse, checked before anything is enqueued. */
int check_sweeps(const vrt_ctx* ctx, int max_steps, float tolerance, float step_min, int n, const void* sweeps, const void* hits) {
    if (!ctx || n < 0 || (n > 0 && (!sweeps || !hits))) return VRT_ERR_INVALID;
    if (max_steps < 1 || max_steps > VRT_MAX_SWEEP_STEPS || !std::isfinite(tolerance) || tolerance < 0.0f) return VRT_ERR_INVALID;
    if (!std::isfinite(step_min) || !(step_min > 0.0f)) return VRT_ERR_INVALID;
    if (!ctx->have_scene) return VRT_ERR_NOT_READY;
    return VRT_OK;
}

/* One launch of n records on the first device.  Touches none of the render's bookkeeping; allocates nothing. */
int enqueue_sweeps(vrt_ctx* ctx, int max_steps, float tolerance, float step_min, int n, const void* sweeps, void* hits, hipStream_t stream) {
    DFrame F;
    const int rc = query_scene(ctx, stream, F);
    if (rc != VRT_OK) return rc;
    const DeviceState& D = ctx->dev[0];
    DSweeps Q;
    memset(&Q, 0, sizeof Q); /* (the whole struct travels as the kernarg) */
    Q.vols = F.vols;
    Q.inst = F.inst;
    Q.n_inst = F.n_inst;
    Q.sweeps = sweeps;
    Q.hits = hits;
    Q.n = n;
    Q.max_steps = max_steps;
    Q.tolerance = tolerance;
    Q.step_min = step_min;
    for (int s = 0; s < VRT_MAX_VOLUMES; s++) {
        Q.material[s] = D.vol[s].material;
        Q.density_scale[s] = ctx->vol[s].density_scale;
    }
    for (int k = 0; k < F.n_inst && k < VRT_MAX_INSTANCES; k++) { /* the resident scene: query_scene has applied a deferred set */
        const vrt_instance& I = ctx->scene.instances[k];
        Q.reach[k] = S::reach(ctx->vol[I.volume_slot].extent, I.scale);
    }
    const dim3 g(((unsigned)n + (unsigned)kSweepThreads - 1u) / (unsigned)kSweepThreads), b(kSweepThreads);
    hipLaunchKernelGGL(sweeps_kernel, g, b, 0, stream, Q);
    HIP_TRY(hipGetLastError());
    return VRT_OK;
}

}  // namespace

}  // namespace vrt

using namespace vrt;

static_assert(sizeof(vrt_sweep) == 32 && sizeof(vrt_sweep_hit) == 64 && offsetof(vrt_sweep_hit, position) == 48,
              "sweeps_kernel reads two and writes four 16-B words per record");

extern "C" {

int vrt_query_sweeps(vrt_ctx* ctx, int max_steps, float tolerance, float step_min, int n, const vrt_sweep* device_sweeps,
                     vrt_sweep_hit* device_hits, void* hip_stream) {
    const int rc = check_sweeps(ctx, max_steps, tolerance, step_min, n, device_sweeps, device_hits);
    if (rc != VRT_OK || n == 0) return rc;
    return enqueue_sweeps(ctx, max_steps, tolerance, step_min, n, device_sweeps, device_hits, static_cast<hipStream_t>(hip_stream));
}

int vrt_query_sweeps_host(vrt_ctx* ctx, int max_steps, float tolerance, float step_min, int n, const vrt_sweep* sweeps, vrt_sweep_hit* hits) {
    int rc = check_sweeps(ctx, max_steps, tolerance, step_min, n, sweeps, hits);
    if (rc != VRT_OK || n == 0) return rc;
    DeviceState& D = ctx->dev[0];
    HIP_TRY(hipSetDevice(D.ordinal));
    const size_t in_bytes = sizeof(vrt_sweep) * (size_t)n, out_bytes = sizeof(vrt_sweep_hit) * (size_t)n;
    rc = ensure_buffer(D.buf[kBufQuery], in_bytes + out_bytes);
    if (rc != VRT_OK) return rc;
    char* base = static_cast<char*>(D.buf[kBufQuery].p);
    HIP_TRY(hipMemcpyAsync(base, sweeps, in_bytes, hipMemcpyHostToDevice, D.stream));
    rc = enqueue_sweeps(ctx, max_steps, tolerance, step_min, n, base, base + in_bytes, D.stream);
    if (rc != VRT_OK) {
        (void)hipStreamSynchronize(D.stream);
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(hits, base + in_bytes, out_bytes, hipMemcpyDeviceToHost, D.stream));
    HIP_TRY(hipStreamSynchronize(D.stream));
    return VRT_OK;
}

}  // extern "C"
