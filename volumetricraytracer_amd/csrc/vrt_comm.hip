/*
 * vrt_comm.hip — the multi-process tile exchange of include/vrt.h (one process per GPU): the RCCL loader, the communicator of a context
 * and the two collectives over it.  Host code only.
 */
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "vrt_context.h"

namespace {

/* RCCL, resolved at run time (librccl is not a link-time dependency: the library loads on hosts without it).  Only what
   the tile exchange needs; signatures from /opt/rocm/include/rccl/rccl.h:164,187,220,260,339,700,722,745,910-920.  The
   function pointers below are declared by hand, so the library's version is checked once: only major version 2 (the API these
   signatures and the value of ncclUint8 = 1, rccl.h:460, belong to) is accepted. */
constexpr int kNcclUint8 = 1;
struct RcclApi {
    typedef struct { char internal[VRT_COMM_ID_BYTES]; } UniqueId;
    int (*GetVersion)(int*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int version = 0;
    int (*GetUniqueId)(UniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*Gather)(const void*, void*, size_t, int /*ncclDataType_t*/, int, void*, hipStream_t) = nullptr;
    bool ok = false;
};
RcclApi* rccl() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return api.ok ? &api : nullptr;
    tried = true;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so"}) /* the copy a host application (e.g. PyTorch) already mapped wins */
        if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL)) != nullptr) break;
    if (!h) return nullptr;
    api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    api.Gather = reinterpret_cast<decltype(api.Gather)>(dlsym(h, "ncclGather"));
    api.GetVersion = reinterpret_cast<decltype(api.GetVersion)>(dlsym(h, "ncclGetVersion"));
    api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(dlsym(h, "ncclGroupStart"));
    api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(dlsym(h, "ncclGroupEnd"));
    api.Send = reinterpret_cast<decltype(api.Send)>(dlsym(h, "ncclSend"));
    api.Recv = reinterpret_cast<decltype(api.Recv)>(dlsym(h, "ncclRecv"));
    api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.GetErrorString && api.Gather && api.GetVersion && api.GroupStart &&
             api.GroupEnd && api.Send && api.Recv;
    if (api.ok) {
        /* NCCL_VERSION_CODE: major * 10000 + minor * 100 + patch from 2.9 on, major * 1000 + minor * 100 + patch before (rccl.h:20) */
        int v = 0;
        const int major = api.GetVersion(&v) == 0 ? (v >= 10000 ? v / 10000 : v / 1000) : -1;
        api.version = v;
        if (major != 2) {
            fprintf(stderr, "[vrt] librccl reports version code %d (major %d): only major version 2 is known to this build; the multi-GPU exchange is disabled\n", v, major);
            api.ok = false;
        }
    }
    return api.ok ? &api : nullptr;
}

}  // namespace

extern "C" {

int vrt_comm_unique_id(void* id_out) {
    if (!id_out) return VRT_ERR_INVALID;
    RcclApi* R = rccl();
    if (!R) return VRT_ERR_UNSUPPORTED;
    RcclApi::UniqueId id;
    const int rc = R->GetUniqueId(&id);
    if (rc != 0) {
        fprintf(stderr, "[vrt] ncclGetUniqueId failed: %s\n", R->GetErrorString(rc));
        return VRT_ERR_HIP;
    }
    memcpy(id_out, id.internal, VRT_COMM_ID_BYTES);
    return VRT_OK;
}

int vrt_comm_init(vrt_ctx* ctx, int world, int rank, const void* id) {
    if (!ctx || !id || world < 1 || rank < 0 || rank >= world || ctx->comm) return VRT_ERR_INVALID;
    RcclApi* R = rccl();
    if (!R) return VRT_ERR_UNSUPPORTED;
    HIP_TRY(hipSetDevice(ctx->dev[0].ordinal));
    RcclApi::UniqueId uid;
    memcpy(uid.internal, id, VRT_COMM_ID_BYTES);
    void* comm = nullptr;
    const int rc = R->CommInitRank(&comm, world, uid, rank);
    if (rc != 0) {
        fprintf(stderr, "[vrt] ncclCommInitRank failed: %s\n", R->GetErrorString(rc));
        return VRT_ERR_HIP;
    }
    ctx->comm = comm;
    ctx->comm_world = world;
    ctx->comm_rank = rank;
    ctx->expect_tile_bytes = ctx->expect_chunk_bytes = 0;
    ctx->sizes_agreed = false;
    return VRT_OK;
}

/* A collective whose ranks disagree about its size does not fail inside RCCL: it waits for ever.  This call (collective, synchronous, a
   setup call) makes the sizes part of the communicator: every rank sends its pair to every rank in one group of 16-byte messages — whose
   size cannot disagree — and compares; afterwards vrt_gather_tiles / vrt_exchange_tiles refuse any other size with VRT_ERR_INVALID before
   they touch RCCL.  0 = that collective is not going to be used (then a call to it is refused).  Call again to change the sizes. */
int vrt_comm_expect_sizes(vrt_ctx* ctx, size_t gather_tile_bytes, size_t exchange_chunk_bytes) {
    if (!ctx || !ctx->comm) return VRT_ERR_NOT_READY;
    RcclApi* R = rccl();
    if (!R) return VRT_ERR_UNSUPPORTED;
    HIP_TRY(hipSetDevice(ctx->dev[0].ordinal));
    const int W = ctx->comm_world;
    struct Pair { unsigned long long tile, chunk; };
    std::vector<Pair> mine((size_t)W, Pair{(unsigned long long)gather_tile_bytes, (unsigned long long)exchange_chunk_bytes}), theirs((size_t)W);
    Pair* d_send = nullptr;
    Pair* d_recv = nullptr;
    hipStream_t st = nullptr;
    int status = VRT_OK;
    do {
        if (hipMalloc(&d_send, sizeof(Pair) * (size_t)W) != hipSuccess || hipMalloc(&d_recv, sizeof(Pair) * (size_t)W) != hipSuccess) { status = VRT_ERR_OOM; break; }
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess ||
            hipMemcpyAsync(d_send, mine.data(), sizeof(Pair) * (size_t)W, hipMemcpyHostToDevice, st) != hipSuccess) { status = VRT_ERR_HIP; break; }
        int rc = R->GroupStart();
        for (int peer = 0; rc == 0 && peer < W; peer++) {
            rc = R->Send(d_send + peer, sizeof(Pair), kNcclUint8, peer, ctx->comm, st);
            if (rc == 0) rc = R->Recv(d_recv + peer, sizeof(Pair), kNcclUint8, peer, ctx->comm, st);
        }
        const int rc_end = R->GroupEnd();
        if (rc != 0 || rc_end != 0) { status = VRT_ERR_HIP; break; }
        if (hipMemcpyAsync(theirs.data(), d_recv, sizeof(Pair) * (size_t)W, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { status = VRT_ERR_HIP; break; }
        for (int peer = 0; peer < W; peer++)
            if (theirs[(size_t)peer].tile != mine[0].tile || theirs[(size_t)peer].chunk != mine[0].chunk) {
                fprintf(stderr, "[vrt] vrt_comm_expect_sizes: rank %d expects tile %llu / chunk %llu bytes, rank %d expects %llu / %llu\n", ctx->comm_rank,
                        mine[0].tile, mine[0].chunk, peer, theirs[(size_t)peer].tile, theirs[(size_t)peer].chunk);
                status = VRT_ERR_INVALID; /* every rank sees the same disagreement and returns the same status */
            }
    } while (false);
    if (st) (void)hipStreamDestroy(st);
    if (d_send) (void)hipFree(d_send);
    if (d_recv) (void)hipFree(d_recv);
    ctx->expect_tile_bytes = status == VRT_OK ? gather_tile_bytes : 0;
    ctx->expect_chunk_bytes = status == VRT_OK ? exchange_chunk_bytes : 0;
    ctx->sizes_agreed = status == VRT_OK;
    return status;
}

int vrt_comm_destroy(vrt_ctx* ctx) {
    if (!ctx) return VRT_ERR_INVALID;
    if (!ctx->comm) return VRT_OK;
    RcclApi* R = rccl();
    if (R) {
        (void)hipSetDevice(ctx->dev[0].ordinal);
        (void)hipDeviceSynchronize();
        (void)R->CommDestroy(ctx->comm);
    }
    ctx->comm = nullptr;
    return VRT_OK;
}

int vrt_gather_tiles(vrt_ctx* ctx, const void* device_tile, void* device_frame_or_null, size_t tile_bytes, int root, void* hip_stream) {
    if (!ctx || !ctx->comm) return VRT_ERR_NOT_READY;
    if (root < 0 || root >= ctx->comm_world || (!device_tile && tile_bytes > 0) ||
        (ctx->comm_rank == root && !device_frame_or_null && tile_bytes > 0))
        return VRT_ERR_INVALID;
    if (ctx->sizes_agreed && tile_bytes != ctx->expect_tile_bytes) return VRT_ERR_INVALID; /* not the size the ranks agreed on: it would wait for ever */
    RcclApi* R = rccl();
    if (!R) return VRT_ERR_UNSUPPORTED;
    HIP_TRY(hipSetDevice(ctx->dev[0].ordinal));
    const int rc = R->Gather(device_tile, device_frame_or_null, tile_bytes, kNcclUint8, root, ctx->comm, static_cast<hipStream_t>(hip_stream));
    if (rc != 0) {
        fprintf(stderr, "[vrt] ncclGather failed: %s\n", R->GetErrorString(rc));
        return VRT_ERR_HIP;
    }
    return VRT_OK;
}

int vrt_exchange_tiles(vrt_ctx* ctx, const void* device_tiles, void* device_recv, size_t chunk_bytes, void* hip_stream) {
    if (!ctx || !ctx->comm) return VRT_ERR_NOT_READY;
    if ((!device_tiles || !device_recv) && chunk_bytes > 0) return VRT_ERR_INVALID;
    if (ctx->sizes_agreed && chunk_bytes != ctx->expect_chunk_bytes) return VRT_ERR_INVALID; /* not the size the ranks agreed on */
    RcclApi* R = rccl();
    if (!R) return VRT_ERR_UNSUPPORTED;
    HIP_TRY(hipSetDevice(ctx->dev[0].ordinal));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    /* one group: every rank's sends and receives progress together (rccl.h:690-691); chunk d of my buffer goes to rank d, chunk
       s of the receive buffer comes from rank s (the own chunk is a device copy inside RCCL) */
    int rc = R->GroupStart();
    for (int peer = 0; rc == 0 && peer < ctx->comm_world; peer++) {
        rc = R->Send(static_cast<const char*>(device_tiles) + (size_t)peer * chunk_bytes, chunk_bytes, kNcclUint8, peer, ctx->comm, stream);
        if (rc == 0) rc = R->Recv(static_cast<char*>(device_recv) + (size_t)peer * chunk_bytes, chunk_bytes, kNcclUint8, peer, ctx->comm, stream);
    }
    const int rc_end = R->GroupEnd();
    if (rc == 0) rc = rc_end;
    if (rc != 0) {
        fprintf(stderr, "[vrt] ncclSend/ncclRecv group failed: %s\n", R->GetErrorString(rc));
        return VRT_ERR_HIP;
    }
    return VRT_OK;
}

}  // extern "C"
