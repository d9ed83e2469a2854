/*
 * grid_device.h — how a kernel reads the dense grid and walks a box of its cells, once, for the calls that only read a slot: the mesh
 * (vrt_mesh.hip), the measure (vrt_measure.hip), the contacts (vrt_contacts.hip) and the point query (vrt_points.hip).  The read side's
 * counterpart of edit_report.h.
 *
 * The unit of work is a run: 64 consecutive cells along y of one (x, z) row of a box of cells, one wave, lane = cell.  Runs are numbered
 * in the grid's storage order (x slowest, then z, then y), so run order followed by lane order IS the order of the cells' keys.  A call
 * that compacts the cells it keeps writes one 16-byte record per run — the ballot's mask and up to two counts —, an exclusive prefix sum
 * over the records turns the counts into the runs' first numbers (launch_run_scan: three launches, block sums, their scan, the
 * records), and a cell's number is its run's first plus a popcount of the mask below its lane: no N^3 index volume, no atomics, and
 * nothing depends on how the device schedules its waves.
 *
 * The kernels have internal linkage: every unit that scans gets its own copies in its code object.
 */
#ifndef VRT_GRID_DEVICE_H
#define VRT_GRID_DEVICE_H

#include <hip/hip_runtime.h>

#include "grid_core.h"
#include "mesh_core.h"
#include "edit_report.h"

namespace vrt {

/* A box of cells (or of samples, each the corner 0 of a cell) of an N^3 grid, in xyz order: its first cell, its cells per axis and how
   many runs of 64 a row along y has. */
struct RunGrid {
    int N;
    int lo[3];
    int n[3];
    int runs_y;
};

/* the box lo..hi, inclusive; no_cells(): hi < lo somewhere */
inline RunGrid run_grid(int N, const int lo_xyz[3], const int hi_xyz[3]) {
    RunGrid G;
    G.N = N;
    for (int a = 0; a < 3; a++) G.lo[a] = lo_xyz[a], G.n[a] = hi_xyz[a] - lo_xyz[a] + 1;
    G.runs_y = (G.n[1] + 63) / 64;
    return G;
}
inline bool no_cells(const RunGrid& G) { return G.n[0] < 1 || G.n[1] < 1 || G.n[2] < 1; }
inline unsigned runs_of(const RunGrid& G) { return (unsigned)G.n[0] * (unsigned)G.n[2] * (unsigned)G.runs_y; }

namespace {

typedef unsigned long long u64;

constexpr int kRunsPerBlock = 4;  /* a pass over the runs: 256 lanes, one run per wave */
constexpr int kScanThreads = 256; /* scan: each lane takes kScanItems consecutive records */
constexpr int kScanItems = 8;
constexpr size_t kRunHeaderBytes = 256; /* the packed totals (and what else a call keeps there), ahead of the block sums */

/* Where lane `lane` of run r sits in the box: the run's row (x, z), its place in the row and the lane's offset along y. */
struct RunPlace {
    unsigned ry;
    int rx, rz, rel_y;
};
__device__ __forceinline__ RunPlace run_place(const RunGrid& G, unsigned r, int lane) {
    RunPlace p;
    p.ry = r % (unsigned)G.runs_y;
    const unsigned t = r / (unsigned)G.runs_y;
    p.rx = (int)(t / (unsigned)G.n[2]), p.rz = (int)(t % (unsigned)G.n[2]);
    p.rel_y = (int)p.ry * 64 + lane;
    return p;
}

/* The cell of lane `lane` of run r (xyz), and whether the row of the box reaches that far. */
__device__ __forceinline__ bool cell_of(const RunGrid& G, unsigned r, int lane, int c[3]) {
    const RunPlace p = run_place(G, r, lane);
    c[0] = G.lo[0] + p.rx;
    c[1] = G.lo[1] + p.rel_y;
    c[2] = G.lo[2] + p.rz;
    return p.rel_y < G.n[1];
}

/* The eight corner values of cell c as the mesh rule reads them (decoded, less iso); every corner must be a sample of the grid.  A
   caller with a template flag for the format passes it as a constant. */
__device__ __forceinline__ void load_corners(const float* __restrict__ dense, int N, const int c[3], float iso, bool texel16, float f[8]) {
    const size_t i0 = vrt_grid::index(N, c[0], c[1], c[2]);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const size_t i = i0 + (size_t)(j & 1) * N * N + (size_t)((j >> 1) & 1) + (size_t)(j >> 2) * N;
        const float s = dense[i];
        f[j] = vrt_mesh::field(vrt_grid::decode(s, texel16), iso);
    }
}

/* The eight decoded taps of cell c, 0 <= c <= N - 2 on every axis, numbered as grid_core.h numbers a cell's corners, for a lane whose
   cell has nothing to do with its neighbours': four y-adjacent pairs, written as adjacent loads for the compiler to merge into 8-byte
   ones (the fp32 bricks' fetch of the march does the same; tools/microbench/gather16.hip checked such loads at 4-byte alignment),
   all eight issued before the first is decoded.  N <= 513, so a sample's index fits 32 bits. */
__device__ __forceinline__ void load_taps(const float* dense, int N, const int c[3], bool texel16, float s[8]) {
    typedef const float __attribute__((address_space(1))) * gfloat_p;
    const unsigned n = (unsigned)N;
    const unsigned at = ((unsigned)c[0] * n + (unsigned)c[2]) * n + (unsigned)c[1];
    const gfloat_p b00 = (gfloat_p)(dense) + at; /* x, z */
    const gfloat_p b01 = b00 + n, b10 = b00 + n * n, b11 = b10 + n;
    s[0] = b00[0], s[2] = b00[1], s[4] = b01[0], s[6] = b01[1];
    s[1] = b10[0], s[3] = b10[1], s[5] = b11[0], s[7] = b11[1];
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = vrt_grid::decode(s[j], texel16);
}

/* The record of a run. */
struct alignas(16) Run {
    u64 mask;          /* bit l: the call keeps cell l of the run */
    unsigned count[2]; /* what the run adds to the call's two numberings (a call with one leaves the second 0); after the scan: the
                          numbers of its first items */
};
__device__ __forceinline__ u64 packed(const Run& r) { return ((u64)r.count[1] << 32) | (u64)r.count[0]; }

/* The number, in the first numbering, of the kept cell at lane `lane` of the run with record rec. */
__device__ __forceinline__ unsigned number_in(const Run& rec, int lane) { return rec.count[0] + (unsigned)__popcll(rec.mask & ((1ull << lane) - 1ull)); }

/* For lane 0 of a run with a mask that is not empty, c its cell — the run's first: x and z are the run's, y runs from the lowest to
   the highest set bit.  The ballot has folded the wave already: the run's two end cells say its box. */
__device__ __forceinline__ void bound_run(EditReport& report, int N, const int c[3], u64 mask) {
    const int y_lo = c[1] + (int)__ffsll((long long)mask) - 1, y_hi = c[1] + 63 - (int)__clzll((long long)mask);
    report.bound(N, c[0], y_lo, c[2]);
    report.bound(N, c[0], y_hi, c[2]);
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

/* The three scan kernels and their launch are templates over the record (Run, deduced) so that only a unit that calls
   launch_run_scan gets the kernels: a plain kernel lands in the code object of every unit that includes its definition.
   sums[b]: the counts of the kScanThreads * kScanItems records of block b, the two packed into one 64-bit word. */
template <class Record>
__global__ __launch_bounds__(kScanThreads) void run_scan_reduce_kernel(const Record* __restrict__ runs, unsigned n_runs, u64* __restrict__ sums) {
    __shared__ u64 wave_sum[kScanThreads / 64];
    const size_t first = ((size_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
    u64 mine = 0ull;
#pragma unroll
    for (int j = 0; j < kScanItems; j++)
        if (first + j < n_runs) mine += packed(runs[first + j]);
    u64 total;
    (void)block_exclusive_scan(mine, total, wave_sum);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

/* One workgroup: sums -> their exclusive prefix sums, *totals = the sum of all. */
template <class Record>
__global__ __launch_bounds__(kScanThreads) void run_scan_sums_kernel(u64* __restrict__ sums, unsigned n_blocks, u64* __restrict__ totals) {
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
    if (threadIdx.x == 0) *totals = carry;
}

/* The records' counts -> the numbers of the runs' first items. */
template <class Record>
__global__ __launch_bounds__(kScanThreads) void run_scan_apply_kernel(Record* __restrict__ runs, unsigned n_runs, const u64* __restrict__ sums) {
    __shared__ u64 wave_sum[kScanThreads / 64];
    const size_t first = ((size_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
    u64 count[kScanItems];
    u64 mine = 0ull;
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        count[j] = first + j < n_runs ? packed(runs[first + j]) : 0ull;
        mine += count[j];
    }
    u64 total;
    u64 at = sums[blockIdx.x] + block_exclusive_scan(mine, total, wave_sum);
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        if (first + j < n_runs) runs[first + j].count[0] = (unsigned)at, runs[first + j].count[1] = (unsigned)(at >> 32);
        at += count[j];
    }
}

/* The scratch of a call that compacts: kRunHeaderBytes whose first word is the packed totals (first numbering in the low half), the
   scan's block sums, and one record per run. */
inline unsigned scan_blocks_of(unsigned n_runs) { return (n_runs + kScanThreads * kScanItems - 1) / (kScanThreads * kScanItems); }
inline size_t sums_bytes(unsigned n_runs) { return ((size_t)scan_blocks_of(n_runs) * sizeof(u64) + 255) / 256 * 256; }
inline size_t run_scratch_bytes(unsigned n_runs) { return kRunHeaderBytes + sums_bytes(n_runs) + (size_t)n_runs * sizeof(Run); }
inline u64* totals_of(void* scratch) { return static_cast<u64*>(scratch); }
inline u64* sums_of(void* scratch) { return reinterpret_cast<u64*>(static_cast<char*>(scratch) + kRunHeaderBytes); }
inline Run* records_of(void* scratch, unsigned n_runs) {
    return reinterpret_cast<Run*>(static_cast<char*>(scratch) + kRunHeaderBytes + sums_bytes(n_runs));
}

/* The records' counts -> the runs' first numbers (a prefix sum in run order), the totals into the scratch's first word. */
template <class Record>
void launch_run_scan(Record* runs, unsigned n_runs, void* scratch, hipStream_t stream) {
    const unsigned n_blocks = scan_blocks_of(n_runs);
    hipLaunchKernelGGL(run_scan_reduce_kernel<Record>, dim3(n_blocks), dim3(kScanThreads), 0, stream, runs, n_runs, sums_of(scratch));
    hipLaunchKernelGGL(run_scan_sums_kernel<Record>, dim3(1), dim3(kScanThreads), 0, stream, sums_of(scratch), n_blocks, totals_of(scratch));
    hipLaunchKernelGGL(run_scan_apply_kernel<Record>, dim3(n_blocks), dim3(kScanThreads), 0, stream, runs, n_runs, sums_of(scratch));
}

}  // namespace

}  // namespace vrt

#endif
