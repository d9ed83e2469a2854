/*
 * edit_report.h — how a kernel that edits a volume tells the host what it wrote: the device side of DBrushSlot (vrt_launch.h), once,
 * for the brushes, fill, redistance, stamp, smooth and the mesh count.
 *
 * A lane keeps an EditReport in registers and adds every sample it writes; at its end the kernel folds the lanes' reports across the
 * wave, and lane 0 of a wave that wrote commits the fold with one atomic per word to one of the kBrushSlots partial records.  The
 * host zeroes the records ahead of the launch (clear_report) and merges them after it.  Plain scalars throughout: nothing here may
 * land in scratch memory.
 */
#ifndef VRT_EDIT_REPORT_H
#define VRT_EDIT_REPORT_H

#include <hip/hip_runtime.h>

#include "vrt_launch.h"

namespace vrt {

static_assert(sizeof(DBrushSlot) == 128 && (kBrushSlots & (kBrushSlots - 1)) == 0, "one line per slot, a power of two of them");

struct EditReport {
    unsigned inv_lo_x = 0u, inv_lo_y = 0u, inv_lo_z = 0u, hi1_x = 0u, hi1_y = 0u, hi1_z = 0u; /* N - lowest, 1 + highest: 0 = none */
    /* The halves of DBrushSlot::counts, the high one as its complement (the samples that do not count there): an op all of whose
       samples count high — fill, stamp, smooth — then carries and folds one counter, the other being the constant 0 (a whole-grid
       stamp runs one sample per lane, so the fold is no small part of a wave's life). */
    unsigned n_low = 0u, n_low_only = 0u;

    /* The box grown to hold sample (x, y, z); nothing is counted (the mesh count reports a box of cells and no counts). */
    __device__ __forceinline__ void bound(int N, int x, int y, int z) {
        inv_lo_x = max(inv_lo_x, (unsigned)(N - x)), inv_lo_y = max(inv_lo_y, (unsigned)(N - y)), inv_lo_z = max(inv_lo_z, (unsigned)(N - z));
        hi1_x = max(hi1_x, (unsigned)(x + 1)), hi1_y = max(hi1_y, (unsigned)(y + 1)), hi1_z = max(hi1_z, (unsigned)(z + 1));
    }

    /* One written sample; `high`: it also counts in the high half of `counts` (what that half means is the op's own). */
    __device__ __forceinline__ void add(int N, int x, int y, int z, bool high) {
        n_low++;
        n_low_only += high ? 0u : 1u;
        bound(N, x, y, z);
    }

    /* This lane's report (a wave's, once folded), which holds something, into the record of `wave_ordinal`: one atomic per word.  The
       ordinal decides only which waves share a record: waves that run together must get different ordinals, or they queue up on one
       line. */
    __device__ __forceinline__ void write(DBrushSlot* __restrict__ slots, unsigned wave_ordinal) const {
        DBrushSlot* slot = slots + (wave_ordinal & (unsigned)(kBrushSlots - 1));
        if (n_low != 0u)
            atomicAdd(&slot->counts, ((unsigned long long)(n_low - n_low_only) << 32) | (unsigned long long)n_low);
        atomicMax(&slot->inv_lo[0], inv_lo_x), atomicMax(&slot->inv_lo[1], inv_lo_y), atomicMax(&slot->inv_lo[2], inv_lo_z);
        atomicMax(&slot->hi1[0], hi1_x), atomicMax(&slot->hi1[1], hi1_y), atomicMax(&slot->hi1[2], hi1_z);
    }

    /* The end of a kernel whose workgroups are whole waves along x, called by every lane: folds the wave, and lane 0 of a wave that
       wrote writes. */
    __device__ __forceinline__ void commit(DBrushSlot* __restrict__ slots, unsigned wave_ordinal) {
        for (int o = 32; o > 0; o >>= 1) {
            n_low += __shfl_xor(n_low, o);
            n_low_only += __shfl_xor(n_low_only, o);
            inv_lo_x = max(inv_lo_x, __shfl_xor(inv_lo_x, o)), inv_lo_y = max(inv_lo_y, __shfl_xor(inv_lo_y, o));
            inv_lo_z = max(inv_lo_z, __shfl_xor(inv_lo_z, o));
            hi1_x = max(hi1_x, __shfl_xor(hi1_x, o)), hi1_y = max(hi1_y, __shfl_xor(hi1_y, o)), hi1_z = max(hi1_z, __shfl_xor(hi1_z, o));
        }
        if ((threadIdx.x & 63u) == 0u && n_low != 0u) write(slots, wave_ordinal);
    }
};

/* Ahead of every launch that reports: all records back to "nothing written". */
inline hipError_t clear_report(DBrushSlot* slots, hipStream_t stream) {
    return hipMemsetAsync(slots, 0, kBrushSlots * sizeof(DBrushSlot), stream);
}

}  // namespace vrt

#endif
