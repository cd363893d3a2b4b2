/* pencilhip.hip — MI355X-native (gfx950) global-transpose engine.
 *
 * Implements include/pencilhip.h: the engine under PencilArrays.jl's
 * Transpositions.transpose! hot path, built from scratch for CDNA4:
 *
 *  - every data movement (pack, unpack, fused local/self copy) is a strided
 *    copy descriptor executed by one of three HIP kernels chosen at plan
 *    time: a vector 1-D copy, a batched linear-runs copy, or an LDS-tiled
 *    N-d transpose (coalesced reads AND writes, 64-wide wavefronts; packed
 *    and wide-element variants for 1-/2-byte and composite elements);
 *  - the subgroup exchange is grouped ncclSend/ncclRecv (RCCL over xGMI) on
 *    the caller's HIP stream — replacing MPI.Isend/Irecv / MPI.Alltoallv!
 *    (Transpositions.jl:419-428, 463-479);
 *  - the self block bypasses the staging buffers entirely (the reference
 *    stages it through recv_buf, :394-404 + :588-606 = 32 B/elem of HBM
 *    traffic; the fused kernel moves 16 B/elem), bit-identical results.
 *
 * Algorithm restated from (0-based, half-open ranges):
 *   split formula           data_ranges.jl:4-9
 *   axes/regions            data_ranges.jl:15-45
 *   to_local                Pencils.jl:579-587
 *   topology / subgroups    MPITopologies.jl:125-136, 208-251
 *   plan + peer blocks      Transpositions.jl:94-119, 282-344, 346-431,
 *                           489-536, 542-552
 *   pack/unpack semantics   Transpositions.jl:554-667 (copy_range! /
 *                           copy_permuted!, perm = permutation(Po)/
 *                           permutation(Pi) at :506)
 *
 * Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC
 *        pencilhip.hip -I../../include -L/opt/rocm/lib -lrccl
 *        -o ../libpencilhip.so
 */

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "pencilhip.h"

/* ================= error handling ================================== */

static thread_local std::string g_err;

extern "C" const char *pa_last_error(void) { return g_err.c_str(); }

static pa_status fail(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define HIP_CHECK(x)                                                         \
    do {                                                                     \
        hipError_t err_ = (x);                                               \
        if (err_ != hipSuccess)                                              \
            return fail("HIP error %s at %s:%d: %s", hipGetErrorName(err_),  \
                        __FILE__, __LINE__, hipGetErrorString(err_));        \
    } while (0)

#define NCCL_CHECK(x)                                                        \
    do {                                                                     \
        ncclResult_t err_ = (x);                                             \
        if (err_ != ncclSuccess)                                             \
            return fail("RCCL error at %s:%d: %s", __FILE__, __LINE__,       \
                        ncclGetErrorString(err_));                           \
    } while (0)

/* ================= kernels ========================================= */

#define MAXND 8

struct DescDev {
    int nd;
    int64_t dims[MAXND], sstr[MAXND], dstr[MAXND];
    int64_t soff, doff, total;
};

/* 1-D contiguous copy, T = 4/8/16-byte word.  The N=1 identity-permutation
 * transpose collapses to this (a straight device copy).  Direct one-element-
 * per-thread mapping: measured 6268 GB/s vs 4729 for a 2048-block
 * grid-stride loop (tools/probe_copy.hip, profiles/r01_probe_copy.txt) —
 * 99.6% of the chip's float4-copy ceiling. */
template <typename T>
__global__ __launch_bounds__(256) void k_copy_1d(const T *__restrict__ src,
                                                 T *__restrict__ dst,
                                                 int64_t n)
{
    /* 2-D grid: the HSA dispatch packet's per-dimension work-item count is
     * 32-bit, so >2^32 threads (e.g. 2048^3 f64 = exactly 2^32 uint4) must
     * split across gridDim.y. */
    const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int64_t i = b * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

/* Nontemporal variant for streams far past the 256 MiB Infinity Cache:
 * bypassing L2/LLC gains ~5% at >=8 GiB payloads but LOSES ~7% when the
 * working set is cache-resident (probe: P1D direct/nt-direct at 128 MiB /
 * 8 GiB / 32 GiB, profiles/r2_probe_kernels8/9.txt) — dispatch gates on
 * payload size. */
typedef unsigned int v4u_nt __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_copy_1d_nt(
    const uint4 *__restrict__ src, uint4 *__restrict__ dst, int64_t n)
{
    const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int64_t i = b * blockDim.x + threadIdx.x;
    if (i < n) {
        v4u_nt v = __builtin_nontemporal_load((const v4u_nt *)&src[i]);
        __builtin_nontemporal_store(v, (v4u_nt *)&dst[i]);
    }
}

/* Batched linear runs: axis 0 contiguous on both sides (coalesced); outer
 * axes strided.  Used for pack (strided window -> contiguous buffer when the
 * fastest axis survives) and its inverse.  Direct mapping (see k_copy_1d).
 * The body is shared by k_copy_linear and the grouped k_group_linear: b is
 * the (entry-local) flat block id. */
template <typename T>
__device__ __forceinline__ void linear_body(const T *__restrict__ src,
                                            T *__restrict__ dst,
                                            const DescDev &d, int64_t b)
{
    const int64_t run = d.dims[0];
    const int64_t idx = b * blockDim.x + threadIdx.x;
    if (idx >= d.total) return;
    int64_t o = idx / run;
    const int64_t i = idx - o * run;
    int64_t so = d.soff + i, doo = d.doff + i;
    for (int a = 1; a < d.nd; a++) {
        const int64_t j = o % d.dims[a];
        o /= d.dims[a];
        so += j * d.sstr[a];
        doo += j * d.dstr[a];
    }
    dst[doo] = src[so];
}

template <typename T>
__global__ __launch_bounds__(256) void k_copy_linear(const T *__restrict__ src,
                                                     T *__restrict__ dst,
                                                     DescDev d)
{
    linear_body<T>(src, dst, d,
                   (int64_t)blockIdx.y * gridDim.x + blockIdx.x);
}

/* Generic gather/scatter (rare fallback: no contiguous axis on either side
 * after normalization, e.g. degenerate unit-extent windows). */
template <typename T>
__global__ __launch_bounds__(256) void k_copy_generic(const T *__restrict__ src,
                                                      T *__restrict__ dst,
                                                      DescDev d)
{
    int64_t idx = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) *
                      blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * gridDim.y * blockDim.x;
    for (; idx < d.total; idx += stride) {
        int64_t rem = idx, so = d.soff, doo = d.doff;
        for (int a = 0; a < d.nd; a++) {
            const int64_t j = rem % d.dims[a];
            rem /= d.dims[a];
            so += j * d.sstr[a];
            doo += j * d.dstr[a];
        }
        dst[doo] = src[so];
    }
}

/* LDS-tiled N-d transpose: src contiguous along axis 0, dst contiguous along
 * axis TA.  Reads coalesced along axis 0 into a padded LDS tile, barrier,
 * writes coalesced along axis TA.  TILE×TILE elements per workgroup,
 * 64×NROWS threads (wave64-shaped).  Remaining axes are batch.
 *
 * The unpack of a permuted pencil (copy_permuted!, Transpositions.jl:588-667)
 * is exactly this kernel; the reference's GPU path does a generic
 * permutedims! plus an extra temporary copy (:651-667 "TODO avoid
 * allocation") — here it is one kernel, no temporary.
 *
 * The body is shared by k_transpose_tile and the grouped k_group_tile: bid
 * is the (entry-local) flat block id, already checked against the block
 * count. */
template <typename T, int TILE_I, int TILE_J, int NROWS, int JCHUNK>
__device__ __forceinline__ void tile_body(
    T (&tile)[TILE_J][TILE_I + 1], const T *__restrict__ src,
    T *__restrict__ dst, const DescDev &d, int ta, int64_t ntile_i,
    int64_t njchunk, int64_t bid)
{
    const int tx = threadIdx.x; /* 0..63  : fast axis */
    const int ty = threadIdx.y; /* 0..NROWS-1 */

    const int64_t t_i = bid % ntile_i;
    int64_t rest = bid / ntile_i;
    const int64_t chunk = rest % njchunk;
    int64_t batch = rest / njchunk;

    /* batch offsets over axes != 0, != ta */
    int64_t so_b = d.soff, do_b = d.doff;
    for (int a = 1; a < d.nd; a++) {
        if (a == ta) continue;
        const int64_t j = batch % d.dims[a];
        batch /= d.dims[a];
        so_b += j * d.sstr[a];
        do_b += j * d.dstr[a];
    }

    const int64_t i0 = t_i * TILE_I; /* along axis 0 */
    const int64_t ni = d.dims[0] - i0 < TILE_I ? d.dims[0] - i0 : TILE_I;

    /* sweep JCHUNK consecutive j-tiles with one workgroup: its reads walk
     * one contiguous src region and each of its TILE_I output rows is
     * written as a sequential stream (probe-measured +1.5% over one tile
     * per WG at the real 1024^3-permuted shape, profiles/probe_ab). */
    for (int jt = 0; jt < JCHUNK; jt++) {
        const int64_t j0 = (chunk * JCHUNK + jt) * TILE_J; /* along ta */
        if (j0 >= d.dims[ta]) break;
        const int64_t nj = d.dims[ta] - j0 < TILE_J ? d.dims[ta] - j0 : TILE_J;

        /* load: lanes sweep axis 0 (src-contiguous), rows sweep axis ta */
        {
            const int64_t base = so_b + i0 /* *1 */ + j0 * d.sstr[ta];
            for (int j = ty; j < nj; j += NROWS) {
                const int64_t row = base + (int64_t)j * d.sstr[ta];
                for (int i = tx; i < ni; i += 64)
                    tile[j][i] = src[row + i];
            }
        }
        __syncthreads();
        /* store: lanes sweep axis ta (dst-contiguous), rows sweep axis 0 */
        {
            const int64_t base = do_b + j0 /* *1 */ + i0 * d.dstr[0];
            for (int i = ty; i < ni; i += NROWS) {
                const int64_t row = base + (int64_t)i * d.dstr[0];
                for (int j = tx; j < nj; j += 64)
                    dst[row + j] = tile[j][i];
            }
        }
        __syncthreads(); /* before the next tile reuses the LDS */
    }
}

template <typename T, int TILE_I, int TILE_J, int NROWS, int JCHUNK>
__global__ __launch_bounds__(64 * NROWS) void k_transpose_tile(
    const T *__restrict__ src, T *__restrict__ dst, DescDev d, int ta,
    int64_t ntile_i, int64_t njchunk, int64_t nblocks)
{
    __shared__ T tile[TILE_J][TILE_I + 1];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    tile_body<T, TILE_I, TILE_J, NROWS, JCHUNK>(tile, src, dst, d, ta,
                                                ntile_i, njchunk, bid);
}

/* The 16-B store of the vector-store tile under its cache policy: plain, or
 * nontemporal (STREAM, see tile_vs_body). */
template <bool STREAM>
__device__ __forceinline__ void vs_store16(void *p, uint4 q)
{
    if (STREAM) {
        v4u_nt v = {q.x, q.y, q.z, q.w};
        __builtin_nontemporal_store(v, (v4u_nt *)p);
    } else {
        *(uint4 *)p = q;
    }
}

/* LDS-tiled transpose with VECTOR (16-B) STORES: 64(i) x 128(j) tile, each
 * lane storing a j-pair as one uint4 — 1024-B write bursts per instruction.
 * Interleaved-median probe (profiles/r2_probe_kernels*.txt): +1.5-1.8% over
 * the scalar 128x64 sweep at the 1024^3-permuted shape (write path is
 * L2-writeback-bound, wider bursts per instruction help where wider tiles
 * do not).  8-byte elements only; caller guarantees every dst stride
 * (except the unit ta axis) and the dst offset are EVEN and the dst base
 * pointer is 16-B aligned, so every vector store is aligned.  Tail j-tiles
 * (nj < TJ or odd) take a scalar epilogue.  Body shared with the grouped
 * k_group_tile_vs, like tile_body.
 *
 * STREAM: nontemporal loads AND nontemporal 16-B vector stores, for payloads
 * far past the caches (select_kernel() gates on payload bytes, like
 * k_copy_1d_nt).  Cache-policy probe at the headline shape, 24 interleaved
 * rounds (tools/probe_stream_tile.hip, profiles/stream_tile_probe.txt): plain
 * 5737 GB/s median, nt stores alone 5842, nt loads alone 5558 (a loss), both
 * 5938 (min 5880 above the control's max 5814).  Write-through (sc1, sc0 sc1)
 * stores measured no better than nt (5837 / 5821 alone, 5908 / 5909 with nt
 * loads) and did not lift the one-direction write-pattern ceiling, and a
 * strided sweep lost 3-5% under every policy, so neither is in the kernel.
 * The two axes travel as ONE policy because neither holds alone: nt loads
 * alone lose at the headline shape and nt stores alone lose at 2 GiB.  On the
 * benchmark's headline the stores alone add 22 GiB/s and the loads 9 more,
 * each above the parent's run-to-run spread of 5 (profiles/
 * stream_tile_bench.txt).  The odd-tail and partial-tile scalar stores stay
 * plain. */
template <typename T, int TI, int TJ, int NROWS, int JCHUNK,
          bool STREAM = false>
__device__ __forceinline__ void tile_vs_body(
    T (&tile)[TI][TJ + 2], const T *__restrict__ src, T *__restrict__ dst,
    const DescDev &d, int ta, int64_t ntile_i, int64_t njchunk, int64_t bid)
{
    static_assert(sizeof(T) == 8, "vector-store tile is 8-byte-elem only");
    const int tx = threadIdx.x;
    const int ty = threadIdx.y;

    const int64_t t_i = bid % ntile_i;
    int64_t rest = bid / ntile_i;
    const int64_t chunk = rest % njchunk;
    int64_t batch = rest / njchunk;

    int64_t so_b = d.soff, do_b = d.doff;
    for (int a = 1; a < d.nd; a++) {
        if (a == ta) continue;
        const int64_t j = batch % d.dims[a];
        batch /= d.dims[a];
        so_b += j * d.sstr[a];
        do_b += j * d.dstr[a];
    }

    const int64_t i0 = t_i * TI;
    const int64_t ni = d.dims[0] - i0 < TI ? d.dims[0] - i0 : TI;

    for (int jt = 0; jt < JCHUNK; jt++) {
        const int64_t j0 = (chunk * JCHUNK + jt) * TJ;
        if (j0 >= d.dims[ta]) break;
        const int64_t nj = d.dims[ta] - j0 < TJ ? d.dims[ta] - j0 : TJ;

        {
            const int64_t base = so_b + i0 + j0 * d.sstr[ta];
            for (int j = ty; j < nj; j += NROWS) {
                const int64_t row = base + (int64_t)j * d.sstr[ta];
                for (int i = tx; i < ni; i += 64)
                    tile[i][j] = STREAM
                                     ? __builtin_nontemporal_load(&src[row + i])
                                     : src[row + i];
            }
        }
        __syncthreads();
        {
            const int64_t base = do_b + j0 + i0 * d.dstr[0];
            const int64_t njv = nj & ~(int64_t)1; /* even part */
            for (int i = ty; i < ni; i += NROWS) {
                T *row = dst + base + (int64_t)i * d.dstr[0];
                for (int j2 = 2 * tx; j2 < njv; j2 += 128) {
                    uint4 q;
                    ((T *)&q)[0] = tile[i][j2];
                    ((T *)&q)[1] = tile[i][j2 + 1];
                    vs_store16<STREAM>(&row[j2], q);
                }
                if ((nj & 1) && tx == 0) /* odd tail element */
                    row[nj - 1] = tile[i][nj - 1];
            }
        }
        __syncthreads();
    }
}

template <typename T, int TI, int TJ, int NROWS, int JCHUNK>
__global__ __launch_bounds__(64 * NROWS) void k_transpose_tile_vs(
    const T *__restrict__ src, T *__restrict__ dst, DescDev d, int ta,
    int64_t ntile_i, int64_t njchunk, int64_t nblocks)
{
    /* TRANSPOSED LDS layout (tile[i][j], +2 pad): the store phase reads
     * 16 B of consecutive j per lane — one wide conflict-free LDS read.
     * The original tile[j][i] layout measured 0.6 LDS-conflict cycles per
     * active cycle (lane-pair row-strided reads); this layout removes them
     * and wins the interleaved A/B by a small margin (probe vs2 p2,
     * profiles/r2_probe_vs2*.txt). */
    __shared__ T tile[TI][TJ + 2];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    tile_vs_body<T, TI, TJ, NROWS, JCHUNK>(tile, src, dst, d, ta, ntile_i,
                                           njchunk, bid);
}

/* The streaming form (tile_vs_body's STREAM policy) under a name of its own,
 * like k_copy_1d_nt: the plain kernel's symbols, and with them its rows in
 * profiles and in the compiler's resource report, stay what they were. */
template <typename T, int TI, int TJ, int NROWS, int JCHUNK>
__global__ __launch_bounds__(64 * NROWS) void k_transpose_tile_vs_nt(
    const T *__restrict__ src, T *__restrict__ dst, DescDev d, int ta,
    int64_t ntile_i, int64_t njchunk, int64_t nblocks)
{
    __shared__ T tile[TI][TJ + 2];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    tile_vs_body<T, TI, TJ, NROWS, JCHUNK, true>(tile, src, dst, d, ta,
                                                 ntile_i, njchunk, bid);
}

/* LDS-tiled transpose for 1- and 2-byte elements with PACKED (8-B) global
 * accesses on both sides.  V = 8/sizeof(T) elements per access.  Each lane
 * owns a VxV micro-block: it loads V rows (consecutive ta) of 8 B of
 * consecutive axis-0 elements, transposes the block in registers, and
 * writes V 8-B LDS words, each holding V consecutive ta elements of one
 * axis-0 row.  The store phase reads one 8-B LDS word per lane and stores it
 * as 8 B of consecutive ta elements — no 1-/2-byte global access on the
 * aligned path.  The caller guarantees that soff, doff and every stride
 * except the two unit ones are multiples of V and both base pointers are
 * 8-B aligned, so every wide access is aligned.  Micro-blocks cut by the
 * tile edge (extents that are no multiple of V) load and store element by
 * element inside the same kernel.
 *
 * LDS layout: row i holds TJ/V 8-B words; word column jb is stored at
 * jb ^ ((i/V) % (TJ/V)), no padding.  Expected bank-conflict degree: none.
 * Write (8-B LDS store, 16-lane groups, 32 banks): the 16 lanes of a group
 * hold 16 consecutive i-blocks of one jb, the row pitch is a multiple of
 * 32 dwords, so the XOR spreads them over 16 distinct dword pairs.  Read
 * (8-B LDS load, 32-lane groups, 64 banks): a group reads 256 contiguous
 * bytes (one 2-byte row or two adjacent 1-byte rows), each word once. */
template <typename T, int TI, int TJ, int NTHR>
__global__ __launch_bounds__(NTHR) void k_transpose_tile_pk(
    const T *__restrict__ src, T *__restrict__ dst, DescDev d, int ta,
    int64_t ntile_i, int64_t ntile_j, int64_t nblocks)
{
    static_assert(sizeof(T) == 1 || sizeof(T) == 2, "packed tile: 1/2-byte");
    constexpr int V = 8 / (int)sizeof(T);
    constexpr int B = 8 * (int)sizeof(T); /* bits per element */
    constexpr int NBI = TI / V, NBJ = TJ / V;
    static_assert(TI % V == 0 && TJ % V == 0, "tile must be whole blocks");
    static_assert(NBI % 16 == 0 && NBJ % 16 == 0 && (NBJ & (NBJ - 1)) == 0,
                  "bank analysis assumes 16-block groups, pow2 columns");
    static_assert((NBI * NBJ) % NTHR == 0 && (TI * NBJ) % NTHR == 0,
                  "whole passes per workgroup");
    constexpr uint64_t EMASK = ((uint64_t)1 << B) - 1;

    __shared__ uint64_t tile[TI * NBJ];

    const int tid = threadIdx.x;
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int64_t t_i = bid % ntile_i;
    int64_t rest = bid / ntile_i;
    const int64_t t_j = rest % ntile_j;
    int64_t batch = rest / ntile_j;

    int64_t so_b = d.soff, do_b = d.doff;
    for (int a = 1; a < d.nd; a++) {
        if (a == ta) continue;
        const int64_t j = batch % d.dims[a];
        batch /= d.dims[a];
        so_b += j * d.sstr[a];
        do_b += j * d.dstr[a];
    }

    const int64_t i0 = t_i * TI;
    const int ni = (int)(d.dims[0] - i0 < TI ? d.dims[0] - i0 : TI);
    const int64_t j0 = t_j * TJ;
    const int nj = (int)(d.dims[ta] - j0 < TJ ? d.dims[ta] - j0 : TJ);

    /* load + in-register transpose + LDS write, one micro-block per pass */
    {
        const int64_t sj = d.sstr[ta];
        const T *base = src + so_b + i0 + j0 * sj;
#pragma unroll
        for (int it = 0; it < NBI * NBJ / NTHR; it++) {
            const int mb = tid + it * NTHR;
            const int bi = mb % NBI, bj = mb / NBI;
            const int ib = bi * V, jb = bj * V;
            if (ib >= ni || jb >= nj) continue; /* never read back */
            uint64_t in[V];
            const T *p = base + (int64_t)jb * sj + ib;
            if (ib + V <= ni && jb + V <= nj) {
#pragma unroll
                for (int r = 0; r < V; r++)
                    in[r] = *(const uint64_t *)(p + (int64_t)r * sj);
            } else { /* block cut by the tile edge: element loads */
#pragma unroll
                for (int r = 0; r < V; r++) {
                    uint64_t w = 0;
                    if (jb + r < nj) {
#pragma unroll
                        for (int k = 0; k < V; k++)
                            if (ib + k < ni)
                                w |= (uint64_t)p[(int64_t)r * sj + k]
                                     << (k * B);
                    }
                    in[r] = w;
                }
            }
            const int col = bj ^ (bi & (NBJ - 1));
#pragma unroll
            for (int k = 0; k < V; k++) {
                uint64_t o = 0;
#pragma unroll
                for (int r = 0; r < V; r++)
                    o |= ((in[r] >> (k * B)) & EMASK) << (r * B);
                tile[(ib + k) * NBJ + col] = o;
            }
        }
    }
    __syncthreads();
    /* store: lanes sweep 8-B words along ta, passes sweep axis 0 */
    {
        const int64_t di = d.dstr[0];
        T *base = dst + do_b + j0 + i0 * di;
#pragma unroll 4
        for (int it = 0; it < TI * NBJ / NTHR; it++) {
            const int c = tid + it * NTHR;
            const int bj = c % NBJ, i = c / NBJ;
            const int jb = bj * V;
            if (i >= ni || jb >= nj) continue;
            const uint64_t v = tile[i * NBJ + (bj ^ ((i / V) & (NBJ - 1)))];
            T *p = base + (int64_t)i * di + jb;
            if (jb + V <= nj) {
                *(uint64_t *)p = v;
            } else { /* ta tail shorter than one word: element stores */
#pragma unroll
                for (int r = 0; r < V; r++)
                    if (jb + r < nj) p[r] = (T)(v >> (r * B));
            }
        }
    }
}

/* LDS-tiled transpose for WIDE elements: an element is m words of WordT
 * (components fastest), e.g. 3 x f64 = three 8-B words.  The descriptor is
 * in ELEMENT units; the tile is ti x tj elements (runtime, chosen per
 * element size by wide_tile_shape()).
 *
 * Load: each tile row along ta is ni*m contiguous src words; lanes sweep the
 * word index q and write LDS word j*pitch + q (consecutive, conflict-free).
 * Store: each tile row along axis 0 is nj*m contiguous dst words; lane q
 * writes word q%m of element j = q/m, read from LDS word
 * j*pitch + i*m + q%m = q + j*(pitch-m) + i*m.  The host picks
 * pitch == m (mod 256/sizeof(WordT)), so consecutive lanes read consecutive
 * LDS words modulo the 256-B bank span: no bank conflicts in either phase.
 *
 * M > 0 is the compile-time words-per-element (M = 3: vectors of three, the
 * common case — q/3 is a constant multiply); M == 0 takes m at runtime and
 * divides with the host-computed magic = ceil(2^32/m), exact for q < 2^26. */
template <typename WordT, int M>
__global__ __launch_bounds__(256) void k_transpose_tile_wide(
    const WordT *__restrict__ src, WordT *__restrict__ dst, DescDev d, int ta,
    int m_rt, uint32_t magic, int ti, int tj, int pitch, int64_t ntile_i,
    int64_t ntile_j, int64_t nblocks)
{
    extern __shared__ uint4 wide_lds[];
    WordT *tile = (WordT *)wide_lds;
    constexpr int NR = 4;

    const int tx = threadIdx.x; /* 0..63 */
    const int ty = threadIdx.y; /* 0..NR-1 */
    const int m = M > 0 ? M : m_rt;

    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int64_t t_i = bid % ntile_i;
    int64_t rest = bid / ntile_i;
    const int64_t t_j = rest % ntile_j;
    int64_t batch = rest / ntile_j;

    int64_t so_b = d.soff, do_b = d.doff;
    for (int a = 1; a < d.nd; a++) {
        if (a == ta) continue;
        const int64_t j = batch % d.dims[a];
        batch /= d.dims[a];
        so_b += j * d.sstr[a];
        do_b += j * d.dstr[a];
    }

    const int64_t i0 = t_i * ti;
    const int ni = (int)(d.dims[0] - i0 < ti ? d.dims[0] - i0 : ti);
    const int64_t j0 = t_j * tj;
    const int nj = (int)(d.dims[ta] - j0 < tj ? d.dims[ta] - j0 : tj);

    /* load: lanes sweep the words of one src row, rows sweep ta */
    {
        const int64_t sj = d.sstr[ta];
        const WordT *base = src + (so_b + i0 + j0 * sj) * m;
        const int nw = ni * m;
        for (int j = ty; j < nj; j += NR) {
            const WordT *row = base + (int64_t)j * sj * m;
            WordT *trow = tile + j * pitch;
            for (int q = tx; q < nw; q += 64) trow[q] = row[q];
        }
    }
    __syncthreads();
    /* store: lanes sweep the words of one dst row, rows sweep axis 0 */
    {
        const int64_t di = d.dstr[0];
        WordT *base = dst + (do_b + j0 + i0 * di) * m;
        const int nw = nj * m;
        const int skip = pitch - m;
        for (int i = ty; i < ni; i += NR) {
            WordT *row = base + (int64_t)i * di * m;
            const WordT *tcol = tile + i * m;
            for (int q = tx; q < nw; q += 64) {
                const int j = M > 0 ? q / M : (int)__umulhi((uint32_t)q, magic);
                row[q] = tcol[q + j * skip];
            }
        }
    }
}

/* ---- grouped kernels: one launch over a table of descriptors ----------
 *
 * A stage of a multi-field transpose (every pack, or every unpack, of every
 * field) is a table of entries in device memory; one launch covers all
 * entries that run the same kernel instance.  The flat block ids of the
 * launch are split among the entries: entry e owns [first[e], first[e+1]).
 * A workgroup finds its entry by a binary search over `first` and then runs
 * the body of the single-descriptor kernel on its entry-local block id.
 *
 * The search reads only blockIdx, gridDim and kernel arguments, so the entry
 * index is the same for every lane; readfirstlane states that to the
 * compiler, which keeps the index, the entry's address and every descriptor
 * field it loads on scalar registers. */
struct GEntry {
    DescDev d;       /* offsets relative to src/dst, in kernel words */
    const void *src; /* base pointers baked in: the table is per array set */
    void *dst;
    int ta;                   /* tile kernels */
    int64_t ntile_i, njchunk; /* tile kernels */
};

__device__ __forceinline__ int group_find(const int64_t *__restrict__ first,
                                          int nent, int64_t bid)
{
    int lo = 0, hi = nent; /* first[lo] <= bid < first[hi] */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= bid)
            lo = mid;
        else
            hi = mid;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

/* COPY_1D and LINEAR entries of one word size (a 1-D copy is a linear copy
 * with no outer axes) */
template <typename T>
__global__ __launch_bounds__(256) void k_group_linear(
    const int64_t *__restrict__ first, const GEntry *__restrict__ ent,
    int nent, int64_t nblocks)
{
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int e = group_find(first, nent, bid);
    const GEntry &g = ent[e];
    linear_body<T>((const T *)g.src, (T *)g.dst, g.d, bid - first[e]);
}

template <typename T, int TILE_I, int TILE_J, int NROWS>
__global__ __launch_bounds__(64 * NROWS) void k_group_tile(
    const int64_t *__restrict__ first, const GEntry *__restrict__ ent,
    int nent, int64_t nblocks)
{
    __shared__ T tile[TILE_J][TILE_I + 1];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int e = group_find(first, nent, bid);
    const GEntry &g = ent[e];
    tile_body<T, TILE_I, TILE_J, NROWS, 1>(tile, (const T *)g.src,
                                           (T *)g.dst, g.d, g.ta, g.ntile_i,
                                           g.njchunk, bid - first[e]);
}

template <typename T, int TI, int TJ, int NROWS>
__global__ __launch_bounds__(64 * NROWS) void k_group_tile_vs(
    const int64_t *__restrict__ first, const GEntry *__restrict__ ent,
    int nent, int64_t nblocks)
{
    __shared__ T tile[TI][TJ + 2];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int e = group_find(first, nent, bid);
    const GEntry &g = ent[e];
    tile_vs_body<T, TI, TJ, NROWS, 1>(tile, (const T *)g.src, (T *)g.dst,
                                      g.d, g.ta, g.ntile_i, g.njchunk,
                                      bid - first[e]);
}

/* ---- grouped zero fill: the destination outside a keep set -------------
 *
 * A truncated transpose (pa_plan_create_keep) writes only the kept indices;
 * the rest of the destination must read +0 for the next FFT.  Each entry is a
 * destination-only window, already scaled by the host to `width`-byte words
 * (select_fill): on a window contiguous along axis 0 a lane stores one word
 * of the run (m = 1, dims[0] = words in the run); on any other window a lane
 * owns one element and stores its m words.  Entry lookup is that of the other
 * grouped kernels, so nd, width, m and every dim and stride sit on scalar
 * registers.  No LDS, no scratch. */
struct GFill {
    int nd;
    int width; /* bytes per store: 16, 8, 4 or 1 */
    int m;     /* stores per lane */
    int pad_;
    int64_t dims[MAXND], dstr[MAXND]; /* lanes per axis; strides in words */
    int64_t doff, total;              /* words; lanes */
    void *dst;
};

template <typename T> __device__ __forceinline__ T zero_word()
{
    return (T)0;
}
template <> __device__ __forceinline__ uint4 zero_word<uint4>()
{
    return make_uint4(0u, 0u, 0u, 0u);
}

template <typename T>
__device__ __forceinline__ void fill_body(const GFill &g, int64_t b)
{
    const int64_t idx = b * blockDim.x + threadIdx.x;
    if (idx >= g.total) return;
    int64_t o = idx, off = g.doff;
    for (int a = 0; a < g.nd; a++) {
        const int64_t j = o % g.dims[a];
        o /= g.dims[a];
        off += j * g.dstr[a];
    }
    T *q = (T *)g.dst + off;
    for (int w = 0; w < g.m; w++) q[w] = zero_word<T>();
}

__device__ __forceinline__ void fill_entry(const GFill &g, int64_t b)
{
    if (g.width == 16)
        fill_body<uint4>(g, b);
    else if (g.width == 8)
        fill_body<uint64_t>(g, b);
    else if (g.width == 4)
        fill_body<uint32_t>(g, b);
    else
        fill_body<uint8_t>(g, b);
}

__global__ __launch_bounds__(256) void k_group_fill(
    const int64_t *__restrict__ first, const GFill *__restrict__ ent,
    int nent, int64_t nblocks)
{
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int e = group_find(first, nent, bid);
    fill_entry(ent[e], bid - first[e]);
}

/* one entry passed by value: pa_device_fill_zero (same body) */
__global__ __launch_bounds__(256) void k_fill(GFill g)
{
    fill_entry(g, (int64_t)blockIdx.y * gridDim.x + blockIdx.x);
}

/* ---- converting kernels: reduced-precision wire ------------------------
 *
 * A wire pair (stored scalar -> wire scalar: f64->f32, f32->f16, f32->bf16)
 * and an op pick the two scalar types of a converting copy: NARROW reads
 * stored and writes wire (packs), WIDEN reads wire and writes stored
 * (unpacks), ROUND reads and writes stored through the wire type (the fused
 * local copy).  Conversions are round-to-nearest-even with subnormals kept
 * (the default kernel float mode); bf16 is done on the bit pattern so the
 * result does not depend on a library.  Descriptors stay in ELEMENT units;
 * an element is ncomp scalars, components fastest. */
struct bf16_t { uint16_t u; };

template <typename D, typename S>
__device__ __forceinline__ D cvt_to(S x)
{
    if constexpr (std::is_same<S, D>::value) {
        return x;
    } else if constexpr (std::is_same<D, bf16_t>::value) {
        const uint32_t u = __float_as_uint(x);
        bf16_t r;
        if ((u & 0x7fffffffu) > 0x7f800000u) /* NaN stays NaN */
            r.u = (uint16_t)((u >> 16) | 0x40u);
        else /* RNE on the pattern; carries into the exponent up to inf */
            r.u = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        return r;
    } else if constexpr (std::is_same<S, bf16_t>::value) {
        return (D)__uint_as_float((uint32_t)x.u << 16);
    } else {
        return (D)x; /* v_cvt: RNE, MODE.denorm keeps subnormals */
    }
}

template <int WIRE> struct WireT;
template <> struct WireT<PA_WIRE_F64_F32> {
    typedef double stored;
    typedef float wire;
};
template <> struct WireT<PA_WIRE_F32_F16> {
    typedef float stored;
    typedef _Float16 wire;
};
template <> struct WireT<PA_WIRE_F32_BF16> {
    typedef float stored;
    typedef bf16_t wire;
};

template <int WIRE, int OP> struct CvtOp {
    typedef typename WireT<WIRE>::stored stored;
    typedef typename WireT<WIRE>::wire wire;
    typedef typename std::conditional<OP == PA_WIRE_WIDEN, wire, stored>::type S;
    typedef typename std::conditional<OP == PA_WIRE_NARROW, wire, stored>::type D;
    static __device__ __forceinline__ D apply(S x)
    {
        if constexpr (OP == PA_WIRE_ROUND)
            return cvt_to<stored>(cvt_to<wire>(x));
        else
            return cvt_to<D>(x);
    }
    /* the tile holds f32 in LDS: the wire type of f64->f32, the stored type
     * of the 16-bit wires (no sub-dword LDS elements, which share banks) */
    static __device__ __forceinline__ float to_lds(S x)
    {
        if constexpr (OP == PA_WIRE_ROUND)
            return cvt_to<float>(cvt_to<wire>(x));
        else
            return cvt_to<float>(x);
    }
    static __device__ __forceinline__ D from_lds(float y)
    {
        return cvt_to<D>(y);
    }
};

template <typename T, int V> struct alignas(sizeof(T) * V) VecT { T v[V]; };

/* Linear runs with conversion: axis 0 contiguous on both sides.  The
 * descriptor is in units of V SCALARS (the host folded ncomp into axis 0 and
 * checked that every access of V scalars is naturally aligned on both
 * sides); a lane converts V consecutive scalars per access.  The body is
 * shared by k_cvt_linear and the grouped k_group_cvt_linear: b is the
 * (entry-local) flat block id. */
template <int WIRE, int OP, int V>
__device__ __forceinline__ void cvt_linear_body(const void *__restrict__ src_,
                                                void *__restrict__ dst_,
                                                const DescDev &d, int64_t b)
{
    typedef CvtOp<WIRE, OP> C;
    typedef VecT<typename C::S, V> SV;
    typedef VecT<typename C::D, V> DV;
    const SV *__restrict__ src = (const SV *)src_;
    DV *__restrict__ dst = (DV *)dst_;
    const int64_t run = d.dims[0];
    const int64_t idx = b * blockDim.x + threadIdx.x;
    if (idx >= d.total) return;
    int64_t o = idx / run;
    const int64_t i = idx - o * run;
    int64_t so = d.soff + i, doo = d.doff + i;
    for (int a = 1; a < d.nd; a++) {
        const int64_t j = o % d.dims[a];
        o /= d.dims[a];
        so += j * d.sstr[a];
        doo += j * d.dstr[a];
    }
    const SV in = src[so];
    DV out;
#pragma unroll
    for (int k = 0; k < V; k++) out.v[k] = C::apply(in.v[k]);
    dst[doo] = out;
}

template <int WIRE, int OP, int V>
__global__ __launch_bounds__(256) void k_cvt_linear(
    const void *__restrict__ src_, void *__restrict__ dst_, DescDev d)
{
    cvt_linear_body<WIRE, OP, V>(src_, dst_, d,
                                 (int64_t)blockIdx.y * gridDim.x + blockIdx.x);
}

/* tile of the converting transpose: CVT_TILE_TJ elements along ta, and along
 * axis 0 as many elements as give rows of about CVT_TILE_ROW scalars (both
 * overridable at build time for shape probes; 64 x 128 measured) */
#ifndef CVT_TILE_TJ
#define CVT_TILE_TJ 64
#endif
#ifndef CVT_TILE_ROW
#define CVT_TILE_ROW 128
#endif
__host__ __device__ constexpr int cvt_tile_ti(int nc)
{
    return CVT_TILE_ROW / nc;
}
__host__ __device__ constexpr int cvt_tile_pitch(int nc)
{
    /* >= ti*nc and == nc modulo the 32 banks of a 4-byte LDS access, so the
     * store phase's nc-scalar runs land on consecutive banks across the row
     * jump (nc = 1: the classic +1 pad) */
    return nc + ((cvt_tile_ti(nc) - 1) * nc + 31) / 32 * 32;
}

/* LDS-tiled transpose with conversion: src contiguous along axis 0, dst
 * contiguous along axis ta, elements of NC <= 4 scalars.  Laid out like the
 * wide-element tile: a tile row along ta is ni*NC contiguous src scalars,
 * written to LDS at j*PITCH + q; a dst row is nj*NC contiguous scalars, lane
 * q storing component q%NC of element q/NC from LDS j*PITCH + i*NC + q%NC.
 * Both phases are conflict-free (see cvt_tile_pitch).  The conversion is
 * split around the f32 LDS image: to_lds on load, from_lds on store.
 *
 * The body is shared by k_cvt_tile and the grouped k_group_cvt_tile: bid is
 * the (entry-local) flat block id, already checked against the block count;
 * tile is the workgroup's CVT_TILE_TJ * cvt_tile_pitch(NC) floats of LDS. */
template <int WIRE, int OP, int NC>
__device__ __forceinline__ void cvt_tile_body(
    float *tile, const void *__restrict__ src_, void *__restrict__ dst_,
    const DescDev &d, int ta, int64_t ntile_i, int64_t ntile_j, int64_t bid)
{
    typedef CvtOp<WIRE, OP> C;
    typedef typename C::S S;
    typedef typename C::D D;
    constexpr int TI = cvt_tile_ti(NC), TJ = CVT_TILE_TJ, NR = 16;
    constexpr int PITCH = cvt_tile_pitch(NC);
    const S *__restrict__ src = (const S *)src_;
    D *__restrict__ dst = (D *)dst_;

    const int tx = threadIdx.x; /* 0..63 */
    const int ty = threadIdx.y; /* 0..NR-1 */
    const int64_t t_i = bid % ntile_i;
    int64_t rest = bid / ntile_i;
    const int64_t t_j = rest % ntile_j;
    int64_t batch = rest / ntile_j;

    int64_t so_b = d.soff, do_b = d.doff;
    for (int a = 1; a < d.nd; a++) {
        if (a == ta) continue;
        const int64_t j = batch % d.dims[a];
        batch /= d.dims[a];
        so_b += j * d.sstr[a];
        do_b += j * d.dstr[a];
    }

    const int64_t i0 = t_i * TI;
    const int ni = (int)(d.dims[0] - i0 < TI ? d.dims[0] - i0 : TI);
    const int64_t j0 = t_j * TJ;
    const int nj = (int)(d.dims[ta] - j0 < TJ ? d.dims[ta] - j0 : TJ);

    /* load: lanes sweep the scalars of one src row, rows sweep ta */
    {
        const int64_t sj = d.sstr[ta];
        const S *base = src + (so_b + i0 + j0 * sj) * NC;
        const int nw = ni * NC;
        for (int j = ty; j < nj; j += NR) {
            const S *row = base + (int64_t)j * sj * NC;
            float *trow = tile + j * PITCH;
            for (int q = tx; q < nw; q += 64) trow[q] = C::to_lds(row[q]);
        }
    }
    __syncthreads();
    /* store: lanes sweep the scalars of one dst row, rows sweep axis 0 */
    {
        const int64_t di = d.dstr[0];
        D *base = dst + (do_b + j0 + i0 * di) * NC;
        const int nw = nj * NC;
        for (int i = ty; i < ni; i += NR) {
            D *row = base + (int64_t)i * di * NC;
            const float *tcol = tile + i * NC;
            for (int q = tx; q < nw; q += 64) {
                const int j = q / NC;
                row[q] = C::from_lds(tcol[q + j * (PITCH - NC)]);
            }
        }
    }
}

template <int WIRE, int OP, int NC>
__global__ __launch_bounds__(1024) void k_cvt_tile(
    const void *__restrict__ src_, void *__restrict__ dst_, DescDev d, int ta,
    int64_t ntile_i, int64_t ntile_j, int64_t nblocks)
{
    __shared__ float tile[CVT_TILE_TJ * cvt_tile_pitch(NC)];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    cvt_tile_body<WIRE, OP, NC>(tile, src_, dst_, d, ta, ntile_i, ntile_j,
                                bid);
}

/* Grouped forms of the two kernels above (PA_PLAN_GROUP_CVT): one launch
 * over a table of entries of one (op, V) resp. (op) signature, the wire pair
 * and the component count being plan constants.  Entry lookup is that of the
 * other grouped kernels; GEntry serves as is, njchunk carrying ntile_j. */
template <int WIRE, int OP, int V>
__global__ __launch_bounds__(256) void k_group_cvt_linear(
    const int64_t *__restrict__ first, const GEntry *__restrict__ ent,
    int nent, int64_t nblocks)
{
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int e = group_find(first, nent, bid);
    const GEntry &g = ent[e];
    cvt_linear_body<WIRE, OP, V>(g.src, g.dst, g.d, bid - first[e]);
}

template <int WIRE, int OP, int NC>
__global__ __launch_bounds__(1024) void k_group_cvt_tile(
    const int64_t *__restrict__ first, const GEntry *__restrict__ ent,
    int nent, int64_t nblocks)
{
    __shared__ float tile[CVT_TILE_TJ * cvt_tile_pitch(NC)];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int e = group_find(first, nent, bid);
    const GEntry &g = ent[e];
    cvt_tile_body<WIRE, OP, NC>(tile, g.src, g.dst, g.d, g.ta, g.ntile_i,
                                g.njchunk, bid - first[e]);
}

/* Elementwise converting fallback: descriptors with no contiguous axis, and
 * transposable ones with more than 4 components.  Correct and slow. */
template <int WIRE, int OP>
__global__ __launch_bounds__(256) void k_cvt_generic(
    const void *__restrict__ src_, void *__restrict__ dst_, DescDev d, int nc)
{
    typedef CvtOp<WIRE, OP> C;
    const typename C::S *__restrict__ src = (const typename C::S *)src_;
    typename C::D *__restrict__ dst = (typename C::D *)dst_;
    int64_t idx = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) *
                      blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * gridDim.y * blockDim.x;
    const int64_t nscal = d.total * nc;
    for (; idx < nscal; idx += stride) {
        int64_t rem = idx / nc;
        const int64_t c = idx - rem * nc;
        int64_t so = d.soff, doo = d.doff;
        for (int a = 0; a < d.nd; a++) {
            const int64_t j = rem % d.dims[a];
            rem /= d.dims[a];
            so += j * d.sstr[a];
            doo += j * d.dstr[a];
        }
        dst[doo * nc + c] = C::apply(src[so * nc + c]);
    }
}

/* ---- scaling kernels: dest = alpha * T(src) ------------------------------
 *
 * A scaled plan (pa_plan_set_scale) multiplies every real scalar S (float or
 * double) by a = S(alpha) in the pass that writes the destination: the fused
 * local copy and the unpacks.  One IEEE multiply per scalar in the default
 * kernel float mode (round to nearest even, subnormals kept).  The kernels
 * are the converting family's with S on both sides and the multiply in place
 * of the conversion; descriptors stay in ELEMENT units of NC scalars. */
template <typename S, int V>
__device__ __forceinline__ void scale_linear_body(
    const void *__restrict__ src_, void *__restrict__ dst_, const DescDev &d,
    int64_t b, S a)
{
    typedef VecT<S, V> SV;
    const SV *__restrict__ src = (const SV *)src_;
    SV *__restrict__ dst = (SV *)dst_;
    const int64_t run = d.dims[0];
    const int64_t idx = b * blockDim.x + threadIdx.x;
    if (idx >= d.total) return;
    int64_t o = idx / run;
    const int64_t i = idx - o * run;
    int64_t so = d.soff + i, doo = d.doff + i;
    for (int ax = 1; ax < d.nd; ax++) {
        const int64_t j = o % d.dims[ax];
        o /= d.dims[ax];
        so += j * d.sstr[ax];
        doo += j * d.dstr[ax];
    }
    const SV in = src[so];
    SV out;
#pragma unroll
    for (int k = 0; k < V; k++) out.v[k] = in.v[k] * a;
    dst[doo] = out;
}

template <typename S, int V>
__global__ __launch_bounds__(256) void k_scale_linear(
    const void *__restrict__ src_, void *__restrict__ dst_, DescDev d, S a)
{
    scale_linear_body<S, V>(src_, dst_, d,
                            (int64_t)blockIdx.y * gridDim.x + blockIdx.x, a);
}

/* tile of the scaling transpose: SCALE_TILE_TJ elements along ta, and along
 * axis 0 as many elements as give rows of SCALE_TILE_ROWB bytes — the f32
 * shape of the converting tile, and for f64 the same bytes per row and per
 * tile */
#define SCALE_TILE_TJ 64
#define SCALE_TILE_ROWB 512
template <typename S> __host__ __device__ constexpr int scale_tile_ti(int nc)
{
    return SCALE_TILE_ROWB / (int)sizeof(S) / nc;
}
template <typename S> __host__ __device__ constexpr int scale_tile_pitch(int nc)
{
    /* in scalars: >= ti*nc and == nc modulo 32.  A 32-lane half then reads
     * scalar indices congruent to 32 consecutive values: 32 banks of the
     * 32-bank ds_read_b32 for f32 (cvt_tile_pitch), 32 bank PAIRS of the
     * 64-bank ds_read_b64 for f64 */
    return nc + ((scale_tile_ti<S>(nc) - 1) * nc + 31) / 32 * 32;
}

/* LDS-tiled transpose with scaling: the layout of cvt_tile_body with S in
 * LDS; the multiply sits on the store side.  bid is the (entry-local) flat
 * block id, already checked against the block count. */
template <typename S, int NC>
__device__ __forceinline__ void scale_tile_body(
    S *tile, const void *__restrict__ src_, void *__restrict__ dst_,
    const DescDev &d, int ta, int64_t ntile_i, int64_t ntile_j, int64_t bid,
    S a)
{
    constexpr int TI = scale_tile_ti<S>(NC), TJ = SCALE_TILE_TJ, NR = 16;
    constexpr int PITCH = scale_tile_pitch<S>(NC);
    const S *__restrict__ src = (const S *)src_;
    S *__restrict__ dst = (S *)dst_;

    const int tx = threadIdx.x; /* 0..63 */
    const int ty = threadIdx.y; /* 0..NR-1 */
    const int64_t t_i = bid % ntile_i;
    int64_t rest = bid / ntile_i;
    const int64_t t_j = rest % ntile_j;
    int64_t batch = rest / ntile_j;

    int64_t so_b = d.soff, do_b = d.doff;
    for (int ax = 1; ax < d.nd; ax++) {
        if (ax == ta) continue;
        const int64_t j = batch % d.dims[ax];
        batch /= d.dims[ax];
        so_b += j * d.sstr[ax];
        do_b += j * d.dstr[ax];
    }

    const int64_t i0 = t_i * TI;
    const int ni = (int)(d.dims[0] - i0 < TI ? d.dims[0] - i0 : TI);
    const int64_t j0 = t_j * TJ;
    const int nj = (int)(d.dims[ta] - j0 < TJ ? d.dims[ta] - j0 : TJ);

    /* load: lanes sweep the scalars of one src row, rows sweep ta */
    {
        const int64_t sj = d.sstr[ta];
        const S *base = src + (so_b + i0 + j0 * sj) * NC;
        const int nw = ni * NC;
        for (int j = ty; j < nj; j += NR) {
            const S *row = base + (int64_t)j * sj * NC;
            S *trow = tile + j * PITCH;
            for (int q = tx; q < nw; q += 64) trow[q] = row[q];
        }
    }
    __syncthreads();
    /* store: lanes sweep the scalars of one dst row, rows sweep axis 0 */
    {
        const int64_t di = d.dstr[0];
        S *base = dst + (do_b + j0 + i0 * di) * NC;
        const int nw = nj * NC;
        for (int i = ty; i < ni; i += NR) {
            S *row = base + (int64_t)i * di * NC;
            const S *tcol = tile + i * NC;
            for (int q = tx; q < nw; q += 64) {
                const int j = q / NC;
                row[q] = tcol[q + j * (PITCH - NC)] * a;
            }
        }
    }
}

template <typename S, int NC>
__global__ __launch_bounds__(1024) void k_scale_tile(
    const void *__restrict__ src_, void *__restrict__ dst_, DescDev d, int ta,
    int64_t ntile_i, int64_t ntile_j, int64_t nblocks, S a)
{
    __shared__ S tile[SCALE_TILE_TJ * scale_tile_pitch<S>(NC)];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    scale_tile_body<S, NC>(tile, src_, dst_, d, ta, ntile_i, ntile_j, bid, a);
}

/* Grouped forms: one launch over the entries of one V resp. all tile entries
 * of a stage, S and NC being plan constants and alpha a kernel argument, so
 * the tables do not depend on it.  GEntry serves as is, njchunk carrying
 * ntile_j. */
template <typename S, int V>
__global__ __launch_bounds__(256) void k_group_scale_linear(
    const int64_t *__restrict__ first, const GEntry *__restrict__ ent,
    int nent, int64_t nblocks, S a)
{
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int e = group_find(first, nent, bid);
    const GEntry &g = ent[e];
    scale_linear_body<S, V>(g.src, g.dst, g.d, bid - first[e], a);
}

template <typename S, int NC>
__global__ __launch_bounds__(1024) void k_group_scale_tile(
    const int64_t *__restrict__ first, const GEntry *__restrict__ ent,
    int nent, int64_t nblocks, S a)
{
    __shared__ S tile[SCALE_TILE_TJ * scale_tile_pitch<S>(NC)];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int e = group_find(first, nent, bid);
    const GEntry &g = ent[e];
    scale_tile_body<S, NC>(tile, g.src, g.dst, g.d, g.ta, g.ntile_i,
                           g.njchunk, bid - first[e], a);
}

/* Elementwise scaling fallback: descriptors with no contiguous axis, and
 * transposable ones with more than 4 scalars per element. */
template <typename S>
__global__ __launch_bounds__(256) void k_scale_generic(
    const void *__restrict__ src_, void *__restrict__ dst_, DescDev d, int nc,
    S a)
{
    const S *__restrict__ src = (const S *)src_;
    S *__restrict__ dst = (S *)dst_;
    int64_t idx = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) *
                      blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * gridDim.y * blockDim.x;
    const int64_t nscal = d.total * nc;
    for (; idx < nscal; idx += stride) {
        int64_t rem = idx / nc;
        const int64_t c = idx - rem * nc;
        int64_t so = d.soff, doo = d.doff;
        for (int ax = 0; ax < d.nd; ax++) {
            const int64_t j = rem % d.dims[ax];
            rem /= d.dims[ax];
            so += j * d.sstr[ax];
            doo += j * d.dstr[ax];
        }
        dst[doo * nc + c] = src[so * nc + c] * a;
    }
}

/* ---- split / join kernels: vector-valued array <-> scalar fields ---------
 *
 * One side of the copy is an array of structs (AoS): n scalars of type S per
 * element, components fastest, scalar c of element e at n*e + c.  The other
 * side is n separately based scalar fields (SoA), field c holding component
 * c.  SPLIT reads the AoS side and writes the fields, JOIN the reverse.  The
 * descriptor is the ordinary one of ONE component in scalar-element units:
 * its source side addresses the AoS array for a split and the fields for a
 * join.  The field base pointers travel by value. */
#define PA_SOA_TILE_MAX_N 4
#define PA_SOA_TILE_TJ 16
#define PA_SOA_GENERIC_PTRS 8
/* Multiplier policy of the split / join kernels, applied to every scalar
 * word while it sits in a register.  SoaNoMul is the identity: the plain
 * kernels.  SoaMul<R> is the scale of the *_scaled calls: the word is one or
 * two real scalars R (float or double; two make a complex scalar) and every
 * one of them is multiplied once by a, the x * a of scale_linear_body.  The
 * policy is a base of the field pointers and travels with them by value: an
 * empty one leaves the kernel arguments as they were.  The index arithmetic,
 * the grid split and the addressing of a kernel are the same lines under
 * either policy. */
struct SoaNoMul {
    /* static and by reference: the word the caller names, not a copy of it,
     * and no use of the pointer struct's address */
    template <typename W>
    static __device__ __forceinline__ const W &mul(const W &x)
    {
        return x;
    }
};
template <typename R> struct SoaMul {
    R a;
    template <typename W> __device__ __forceinline__ W mul(W x) const
    {
        constexpr int L = (int)(sizeof(W) / sizeof(R));
        static_assert(sizeof(W) == L * sizeof(R) && (L == 1 || L == 2),
                      "a scalar word is one or two real scalars");
        VecT<R, L> r;
        __builtin_memcpy(&r, &x, sizeof(W));
#pragma unroll
        for (int k = 0; k < L; k++) r.v[k] = r.v[k] * a;
        __builtin_memcpy(&x, &r, sizeof(W));
        return x;
    }
};
template <int N, typename M = SoaNoMul> struct SoaPtrs : M { void *p[N]; };

/* Axis 0 contiguous on both sides.  A lane owns V consecutive elements: the
 * N*V AoS scalars are N aligned V-scalar vectors next to each other, and each
 * field gets one V-scalar vector; the interleave between them happens in
 * registers with compile-time indices.  The descriptor is in units of V
 * scalars.  The N AoS accesses of a wave cover one contiguous range of
 * 64*N*V scalars, every byte of it exactly once.
 *
 * The body is shared by k_soa_linear and the grouped k_group_soa_linear: fp
 * points at the N field pointers where they lie (the kernel arguments, or an
 * entry of the grouped table), f is the multiplier policy, b the
 * (entry-local) flat block id. */
template <typename S, int DIR, int N, int V, typename M>
__device__ __forceinline__ void soa_linear_body(void *__restrict__ aos_,
                                                void *const *fp, const M &f,
                                                const DescDev &d, int64_t b)
{
    typedef VecT<S, V> SV;
    const int64_t run = d.dims[0];
    const int64_t idx = b * blockDim.x + threadIdx.x;
    if (idx >= d.total) return;
    int64_t o = idx / run;
    const int64_t i = idx - o * run;
    int64_t so = d.soff + i, doo = d.doff + i;
    for (int ax = 1; ax < d.nd; ax++) {
        const int64_t j = o % d.dims[ax];
        o /= d.dims[ax];
        so += j * d.sstr[ax];
        doo += j * d.dstr[ax];
    }
    SV *aos = (SV *)aos_ + (DIR == PA_SOA_SPLIT ? so : doo) * N;
    const int64_t fo = DIR == PA_SOA_SPLIT ? doo : so;
    S flat[N * V]; /* scalar v*N + c: component c of the lane's element v */
    if (DIR == PA_SOA_SPLIT) {
#pragma unroll
        for (int k = 0; k < N; k++) {
            const SV in = aos[k];
#pragma unroll
            for (int j = 0; j < V; j++) flat[k * V + j] = in.v[j];
        }
#pragma unroll
        for (int k = 0; k < N * V; k++) flat[k] = f.mul(flat[k]);
#pragma unroll
        for (int c = 0; c < N; c++) {
            SV out;
#pragma unroll
            for (int v = 0; v < V; v++) out.v[v] = flat[v * N + c];
            ((SV *)fp[c])[fo] = out;
        }
    } else {
#pragma unroll
        for (int c = 0; c < N; c++) {
            const SV in = ((const SV *)fp[c])[fo];
#pragma unroll
            for (int v = 0; v < V; v++) flat[v * N + c] = in.v[v];
        }
#pragma unroll
        for (int k = 0; k < N * V; k++) flat[k] = f.mul(flat[k]);
#pragma unroll
        for (int k = 0; k < N; k++) {
            SV out;
#pragma unroll
            for (int j = 0; j < V; j++) out.v[j] = flat[k * V + j];
            aos[k] = out;
        }
    }
}

template <typename S, int DIR, int N, int V, typename M = SoaNoMul>
__global__ __launch_bounds__(256) void k_soa_linear(void *__restrict__ aos_,
                                                    SoaPtrs<N, M> f,
                                                    DescDev d)
{
    soa_linear_body<S, DIR, N, V, M>(
        aos_, f.p, f, d, (int64_t)blockIdx.y * gridDim.x + blockIdx.x);
}

/* The permuted case: the source side is contiguous along axis 0, the
 * destination side along axis ta.  One LDS tile of ti (axis 0) x tj (ta)
 * elements x N components; tj is PA_SOA_TILE_TJ.  The AoS side moves rows of
 * ni*N or nj*N contiguous scalars with the word-index sweep of
 * k_transpose_tile_wide, q / N being a constant division.
 *
 * SPLIT: the tile is the wide tile's, word j*pitch + i*N + c, pitch >= ti*N.
 * The AoS load writes consecutive LDS words.  The store puts lane
 * (c, j) = (tx / tj, tx % tj) on field c along ta, so the N components share
 * a wave (N*tj <= 64 lanes); with pitch == N (mod 256/W) its LDS words are
 * i*N + j*N + c modulo the bank span: N*tj different consecutive words, which
 * share a bank only where they wrap the span of 256/W words.
 *
 * JOIN: the tile is planar, word c*plane + j*pitch + i, pitch >= ti.  Each
 * component tile is loaded like tile_body's (lanes along axis 0: consecutive
 * LDS words).  The AoS store reads, at word index q = j*N + c of row i,
 * c*plane + j*pitch + i; with plane == 1 and pitch == N (mod 256/W) that is
 * q + i modulo the bank span: consecutive lanes, consecutive banks.
 *
 * The body is shared by k_soa_tile and the grouped k_group_soa_tile: tile is
 * the workgroup's LDS, fp and f as in soa_linear_body (the split's store
 * picks its field by lane, so the pointers must stay where a lane can index
 * them: a copy in registers would go to scratch), bid the (entry-local) flat
 * block id, already checked against the block count. */
template <typename S, int DIR, int N, typename M>
__device__ __forceinline__ void soa_tile_body(
    S *tile, void *__restrict__ aos_, void *const *fp, const M &f,
    const DescDev &d, int ta, int ti, int pitch, int plane, int64_t ntile_i,
    int64_t ntile_j, int64_t bid)
{
    constexpr int NR = 4;
    constexpr int TJ = PA_SOA_TILE_TJ;
    static_assert(N * TJ <= 64, "the components of a split store share a wave");

    const int tx = threadIdx.x; /* 0..63 */
    const int ty = threadIdx.y; /* 0..NR-1 */

    const int64_t t_i = bid % ntile_i;
    int64_t rest = bid / ntile_i;
    const int64_t t_j = rest % ntile_j;
    int64_t batch = rest / ntile_j;

    int64_t so_b = d.soff, do_b = d.doff;
    for (int a = 1; a < d.nd; a++) {
        if (a == ta) continue;
        const int64_t j = batch % d.dims[a];
        batch /= d.dims[a];
        so_b += j * d.sstr[a];
        do_b += j * d.dstr[a];
    }

    const int64_t i0 = t_i * ti;
    const int ni = (int)(d.dims[0] - i0 < ti ? d.dims[0] - i0 : ti);
    const int64_t j0 = t_j * TJ;
    const int nj = (int)(d.dims[ta] - j0 < TJ ? d.dims[ta] - j0 : TJ);
    const int64_t sj = d.sstr[ta];
    const int64_t di = d.dstr[0];

    if (DIR == PA_SOA_SPLIT) {
        /* load: lanes sweep the words of one AoS row, rows sweep ta */
        {
            const S *base = (const S *)aos_ + (so_b + i0 + j0 * sj) * N;
            const int nw = ni * N;
            for (int j = ty; j < nj; j += NR) {
                const S *row = base + (int64_t)j * sj * N;
                S *trow = tile + j * pitch;
                for (int q = tx; q < nw; q += 64) trow[q] = row[q];
            }
        }
        __syncthreads();
        /* store: lane (c, j) writes field c along ta, rows sweep axis 0 */
        {
            const int c = tx / TJ, j = tx % TJ;
            if (c < N && j < nj) {
                S *dst = (S *)fp[0];
#pragma unroll
                for (int cc = 1; cc < N; cc++)
                    if (c == cc) dst = (S *)fp[cc];
                dst += do_b + j0 + i0 * di + j;
                const S *tcol = tile + j * pitch + c;
                for (int i = ty; i < ni; i += NR)
                    dst[(int64_t)i * di] = f.mul(tcol[i * N]);
            }
        }
    } else {
        /* load: per component, lanes sweep axis 0, rows sweep ta */
        {
            const int64_t fbase = so_b + i0 + j0 * sj;
#pragma unroll
            for (int c = 0; c < N; c++) {
                const S *src = (const S *)fp[c] + fbase;
                for (int j = ty; j < nj; j += NR) {
                    const S *row = src + (int64_t)j * sj;
                    S *trow = tile + c * plane + j * pitch;
                    for (int i = tx; i < ni; i += 64) trow[i] = row[i];
                }
            }
        }
        __syncthreads();
        /* store: lanes sweep the words of one AoS row, rows sweep axis 0 */
        {
            S *base = (S *)aos_ + (do_b + j0 + i0 * di) * N;
            const int nw = nj * N;
            for (int i = ty; i < ni; i += NR) {
                S *row = base + (int64_t)i * di * N;
                for (int q = tx; q < nw; q += 64) {
                    const int j = q / N, c = q - j * N;
                    row[q] = f.mul(tile[c * plane + j * pitch + i]);
                }
            }
        }
    }
}

template <typename S, int DIR, int N, typename M = SoaNoMul>
__global__ __launch_bounds__(256) void k_soa_tile(
    void *__restrict__ aos_, SoaPtrs<N, M> f, DescDev d, int ta, int ti,
    int pitch, int plane, int64_t ntile_i, int64_t ntile_j, int64_t nblocks)
{
    extern __shared__ uint4 soa_lds[];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    soa_tile_body<S, DIR, N, M>((S *)soa_lds, aos_, f.p, f, d, ta, ti, pitch,
                                plane, ntile_i, ntile_j, bid);
}

/* Grouped forms of the two kernels above (PA_PLAN_GROUP_SOA): one launch over
 * a table of entries of one V resp. all tile entries of a stage; S, the
 * direction, N and the multiplier policy are the same for every entry of a
 * stage call.  Entry lookup is that of the other grouped kernels, so the
 * descriptor, the base pointers and the tile shape sit on scalar registers.
 * The multiplier is a kernel argument: the tables do not depend on alpha. */
struct GSoa {
    DescDev d;  /* linear: in units of V scalars; tile: scalars */
    void *aos;  /* base pointers baked in: the table is per array set */
    void *f[PA_SOA_TILE_MAX_N]; /* fields, or the slots of a staging block */
    int ta, ti, pitch, plane;   /* tile kernels */
    int64_t ntile_i, ntile_j;   /* tile kernels */
};

template <typename S, int DIR, int N, int V, typename M>
__global__ __launch_bounds__(256) void k_group_soa_linear(
    const int64_t *__restrict__ first, const GSoa *__restrict__ ent, int nent,
    int64_t nblocks, M m)
{
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int e = group_find(first, nent, bid);
    const GSoa &g = ent[e];
    soa_linear_body<S, DIR, N, V, M>(g.aos, g.f, m, g.d, bid - first[e]);
}

template <typename S, int DIR, int N, typename M>
__global__ __launch_bounds__(256) void k_group_soa_tile(
    const int64_t *__restrict__ first, const GSoa *__restrict__ ent, int nent,
    int64_t nblocks, M m)
{
    extern __shared__ uint4 soa_lds[];
    const int64_t bid = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (bid >= nblocks) return;
    const int e = group_find(first, nent, bid);
    const GSoa &g = ent[e];
    soa_tile_body<S, DIR, N, M>((S *)soa_lds, g.aos, g.f, m, g.d, g.ta, g.ti,
                                g.pitch, g.plane, g.ntile_i, g.ntile_j,
                                bid - first[e]);
}

/* Any other descriptor, any n: one lane per scalar, grid-stride like
 * k_copy_generic.  blockIdx.z is the component within this launch's chunk of
 * at most PA_SOA_GENERIC_PTRS fields, whose first component is c0. */
template <typename S, int DIR, typename M = SoaNoMul>
__global__ __launch_bounds__(256) void k_soa_generic(
    void *__restrict__ aos_, SoaPtrs<PA_SOA_GENERIC_PTRS, M> f, DescDev d,
    int n, int c0)
{
    const int c = blockIdx.z;
    S *fp = (S *)f.p[0];
#pragma unroll
    for (int cc = 1; cc < PA_SOA_GENERIC_PTRS; cc++)
        if (c == cc) fp = (S *)f.p[cc];
    S *aos = (S *)aos_ + c0 + c;
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; idx < d.total; idx += stride) {
        int64_t rem = idx, so = d.soff, doo = d.doff;
        for (int a = 0; a < d.nd; a++) {
            const int64_t j = rem % d.dims[a];
            rem /= d.dims[a];
            so += j * d.sstr[a];
            doo += j * d.dstr[a];
        }
        if (DIR == PA_SOA_SPLIT)
            fp[doo] = f.mul(aos[so * n]);
        else
            aos[doo * n] = f.mul(fp[so]);
    }
}

/* ================= descriptor normalization & dispatch ============= */

struct CopyDescH {
    int nd = 0;
    int64_t dims[MAXND] = {0}, sstr[MAXND] = {0}, dstr[MAXND] = {0};
    int64_t soff = 0, doff = 0;
    int64_t total = 0;
};

static CopyDescH normalize_desc(int nd, const int64_t *dims,
                                const int64_t *sstr, int64_t soff,
                                const int64_t *dstr, int64_t doff)
{
    struct Axis { int64_t dim, ss, ds; };
    std::vector<Axis> ax;
    for (int i = 0; i < nd; i++)
        if (dims[i] != 1) ax.push_back({dims[i], sstr[i], dstr[i]});
    if (ax.empty()) ax.push_back({1, 1, 1});
    std::sort(ax.begin(), ax.end(),
              [](const Axis &a, const Axis &b) { return a.ss < b.ss; });
    std::vector<Axis> m{ax[0]};
    for (size_t i = 1; i < ax.size(); i++) {
        Axis &p = m.back();
        if (ax[i].ss == p.ss * p.dim && ax[i].ds == p.ds * p.dim)
            p.dim *= ax[i].dim;
        else
            m.push_back(ax[i]);
    }
    CopyDescH out;
    out.nd = (int)m.size();
    out.total = 1;
    for (int i = 0; i < out.nd; i++) {
        out.dims[i] = m[i].dim;
        out.sstr[i] = m[i].ss;
        out.dstr[i] = m[i].ds;
        out.total *= m[i].dim;
    }
    out.soff = soff;
    out.doff = doff;
    return out;
}

/* Try to reinterpret a linear-runs descriptor in W-byte words (W >= esz). */
static bool word_scale(const CopyDescH &d, int64_t esz, int64_t W,
                       CopyDescH *out)
{
    if ((d.dims[0] * esz) % W || (d.soff * esz) % W || (d.doff * esz) % W)
        return false;
    for (int a = 1; a < d.nd; a++)
        if ((d.sstr[a] * esz) % W || (d.dstr[a] * esz) % W) return false;
    *out = d;
    out->dims[0] = d.dims[0] * esz / W;
    out->soff = d.soff * esz / W;
    out->doff = d.doff * esz / W;
    for (int a = 1; a < d.nd; a++) {
        out->sstr[a] = d.sstr[a] * esz / W;
        out->dstr[a] = d.dstr[a] * esz / W;
    }
    out->total = out->dims[0];
    for (int a = 1; a < out->nd; a++) out->total *= out->dims[a];
    return true;
}

static DescDev to_dev(const CopyDescH &d)
{
    DescDev o;
    o.nd = d.nd;
    for (int i = 0; i < MAXND; i++) {
        o.dims[i] = i < d.nd ? d.dims[i] : 1;
        o.sstr[i] = i < d.nd ? d.sstr[i] : 0;
        o.dstr[i] = i < d.nd ? d.dstr[i] : 0;
    }
    o.soff = d.soff;
    o.doff = d.doff;
    o.total = d.total;
    return o;
}

/* Exact one-element-per-thread grid (probe-measured fastest for the
 * memory-bound copies: the dispatcher streams blocks, no software loop). */
static int64_t grid_exact(int64_t work_items, int per_block)
{
    int64_t blocks = (work_items + per_block - 1) / per_block;
    if (blocks < 1) blocks = 1;
    return blocks;
}

/* Split a block count into a 2-D grid: the HSA dispatch limit is 2^32-1
 * WORK-ITEMS per grid dimension, so gridDim.x is capped at that / threads
 * and the remainder goes to gridDim.y. */
static pa_status grid2d(int64_t blocks, int threads_per_block, dim3 *out)
{
    const int64_t max_x = 0xFFFFFFFFll / threads_per_block;
    int64_t gx = blocks < max_x ? blocks : max_x;
    int64_t gy = (blocks + gx - 1) / gx;
    if (gy > 0xFFFFFFFFll) return fail("grid too large");
    *out = dim3((uint32_t)gx, (uint32_t)gy);
    return 0;
}

static int grid_for(int64_t work_items, int per_block)
{
    int64_t blocks = grid_exact(work_items, per_block);
    const int64_t cap = 8192; /* generic fallback only */
    if (blocks > cap) blocks = cap;
    return (int)blocks;
}

/* The outcome of the dispatch decision: which kernel runs, on which
 * (possibly word-scaled or byte-ified) descriptor.  select_kernel() is the
 * ONE place the decision is made; launch_sel() only executes it and
 * pa_copy_kernel_kind() only reports it. */
struct KernelSel {
    int kind = PA_KERNEL_NONE;
    int word = 0;      /* bytes per kernel word */
    int byteified = 0; /* went through the byte-ify fallback */
    int sweep = 1;     /* j-tiles swept per workgroup (tile kernels) */
    int stream = 0;    /* TILE_VS: nontemporal loads and vector stores */
    int ta = -1;       /* dst-contiguous axis (tile kernels) */
    int m = 1;         /* words per element (wide tile / word-expanded) */
    int ti = 0, tj = 0, pitch = 0; /* wide tile: shape (elements), LDS row
                                    * pitch (words) */
    CopyDescH d;       /* the descriptor the kernel runs, in `word` units
                        * (wide tile: in ELEMENT units of m words each) */
};

/* sweep depth of the 4-/8-byte tiles: long sweeps win on tall-skinny shapes
 * (+1.5% A/B) but must keep >= ~4k workgroups for occupancy and tail
 * balance on small/batched shapes */
static int sweep_depth(int64_t nti, int64_t ntj, int64_t nbatch)
{
    if (ntj * nti * nbatch >= 32 * 4096 && ntj >= 256) return 32;
    if (ntj * nti * nbatch >= 8 * 4096 && ntj >= 64) return 8;
    return 1;
}

/* Payload bytes from which the vector-store tile streams
 * (pa_set_stream_min_bytes; negative = never).  Probe rows behind the number
 * (profiles/stream_tile_probe.txt, GB/s, control median and max against the
 * streaming median, sweep depth by sweep_depth()):
 *   128 MiB  6482 / 6526  vs 5840   loses (cache-resident)
 *   256 MiB  5158 / 5193  vs 5883   wins
 *   512 MiB  5018 / 5084  vs 5557   wins
 *     1 GiB  5376 / 5441  vs 5803   wins
 *     2 GiB  5640 / 5673  vs 5977   wins
 *     8 GiB  5742 / 5821  vs 5941   wins
 * The streaming median beats the control's max from 256 MiB up; below 512 MiB
 * the gate takes 512 MiB, the k_copy_1d_nt gate. */
static std::atomic<int64_t> g_stream_min_bytes{512ll << 20};

static pa_status select_kernel(const CopyDescH &dn, int64_t esz,
                               const void *src, const void *dst,
                               KernelSel *out)
{
    *out = KernelSel();
    if (dn.total == 0) return 0;

    const bool lin = (dn.sstr[0] == 1 && dn.dstr[0] == 1);
    if (lin) {
        /* widest word dividing the run, every stride/offset in bytes, and
         * both base addresses (a sliced tensor moves the base by one
         * element) */
        const uintptr_t ptrs = (uintptr_t)src | (uintptr_t)dst;
        CopyDescH w;
        int64_t W = 0;
        for (int64_t cand : {16, 8, 4})
            if (cand >= esz || (esz % cand) == 0)
                if ((ptrs & (uintptr_t)(cand - 1)) == 0 &&
                    word_scale(dn, esz, cand, &w)) { W = cand; break; }
        if (!W) { /* odd element size: fall back to bytes */
            if (!word_scale(dn, esz, 1, &w)) return fail("word_scale(1)");
            W = 1;
        }
        out->word = (int)W;
        out->d = w;
        if (w.nd == 1)
            out->kind = (W == 16 && w.total * 16 >= (512ll << 20))
                            ? PA_KERNEL_COPY_1D_NT
                            : PA_KERNEL_COPY_1D;
        else
            out->kind = PA_KERNEL_LINEAR;
        return 0;
    }

    /* transpose case: src-contiguous axis 0, find dst-contiguous axis */
    int ta = -1;
    if (dn.sstr[0] == 1)
        for (int a = 1; a < dn.nd; a++)
            if (dn.dstr[a] == 1) { ta = a; break; }

    const bool pow2 = esz == 1 || esz == 2 || esz == 4 || esz == 8 ||
                      esz == 16;
    if (ta > 0 && pow2) {
        int64_t nbatch = 1;
        for (int a = 1; a < dn.nd; a++)
            if (a != ta) nbatch *= dn.dims[a];
        out->word = (int)esz;
        out->d = dn;
        out->ta = ta;
        /* tile shapes probe-measured on MI355X (profiles/r01_probe_copy*,
         * r2_probe_kernels*): 8-B elements prefer the 64x128 vector-store
         * tile (+1.5-1.8% median) when alignment permits; otherwise (and
         * for 4-B) the scalar 128(i)x64(j) r16 sweep; 16-B: 32x32.
         * 1-/2-B elements take the packed 128x128 tile when every 8-B
         * access is aligned, else the scalar 128x64 tile. */
        if (esz == 8) {
            bool vec_ok = ((dn.doff & 1) == 0) && ((dn.dstr[0] & 1) == 0) &&
                          (((uintptr_t)dst & 15) == 0);
            for (int a2 = 1; a2 < dn.nd && vec_ok; a2++)
                if (a2 != ta && (dn.dstr[a2] & 1)) vec_ok = false;
            if (vec_ok) {
                out->kind = PA_KERNEL_TILE_VS;
                out->sweep = sweep_depth((dn.dims[0] + 63) / 64,
                                         (dn.dims[ta] + 127) / 128, nbatch);
                const int64_t smin = g_stream_min_bytes.load();
                out->stream = smin >= 0 && dn.total * 8 >= smin;
                return 0;
            }
        }
        if (esz <= 2) {
            const int64_t V = 8 / esz;
            bool pk_ok = (dn.soff % V == 0) && (dn.doff % V == 0) &&
                         (((uintptr_t)src & 7) == 0) &&
                         (((uintptr_t)dst & 7) == 0) &&
                         (dn.dstr[0] % V == 0);
            for (int a2 = 1; a2 < dn.nd && pk_ok; a2++) {
                if (dn.sstr[a2] % V) pk_ok = false;
                if (a2 != ta && dn.dstr[a2] % V) pk_ok = false;
            }
            out->kind = pk_ok ? PA_KERNEL_TILE_PK : PA_KERNEL_TILE;
            return 0;
        }
        out->kind = PA_KERNEL_TILE;
        if (esz == 8 || esz == 4)
            out->sweep = sweep_depth((dn.dims[0] + 127) / 128,
                                     (dn.dims[ta] + 63) / 64, nbatch);
        return 0;
    }

    /* generic fallback */
    if (pow2) {
        out->kind = PA_KERNEL_GENERIC;
        out->word = (int)esz;
        out->d = dn;
        return 0;
    }

    /* any other element size (the reference allows arbitrary isbits
     * element types): byte-ify — prepend a stride-1 axis of esz bytes,
     * which makes the descriptor linear-copyable at byte granularity
     * (slow for tiny elements, always correct) */
    {
        if (dn.nd + 1 > MAXND) return fail("too many dims to byte-ify");
        int64_t dims[MAXND + 1], ss[MAXND + 1], ds[MAXND + 1];
        dims[0] = esz;
        ss[0] = 1;
        ds[0] = 1;
        for (int a = 0; a < dn.nd; a++) {
            dims[a + 1] = dn.dims[a];
            ss[a + 1] = dn.sstr[a] * esz;
            ds[a + 1] = dn.dstr[a] * esz;
        }
        CopyDescH b = normalize_desc(dn.nd + 1, dims, ss, dn.soff * esz, ds,
                                     dn.doff * esz);
        pa_status st = select_kernel(b, 1, src, dst, out);
        out->byteified = 1;
        return st;
    }
}

/* ---- composite elements: ncomp scalars of ssz bytes, components fastest */

/* Tile shape (elements) of the wide tile per element size B: 16 rows along
 * ta, and along axis 0 the largest power of two (16..256) whose row is at
 * most 1536 bytes — a ~24 KiB tile, six or more workgroups per CU.
 * Probe-measured on MI355X at the 512^3 permuted shape over ti in 16..256
 * and tj in 8..64 for B = 6, 12, 24, 48 (composite elements):
 * the best or within 2% of the best shape for each B; square 32x32 / 64x64
 * tiles were 15-45% slower. */
static void wide_tile_shape(int64_t B, int *ti, int *tj)
{
    int t = 256;
    while (t > 16 && t * B > 1536) t >>= 1;
    *ti = t;
    *tj = 16;
}

#define PA_WIDE_MAX_BYTES 64

/* the (scalar_size, ncomp) pairs the engine accepts: any positive size for
 * one scalar per element, a power of two <= 16 for composite elements */
static pa_status check_comp(int64_t scalar_size, int64_t ncomp)
{
    if (ncomp < 1) return fail("invalid ncomp %lld", (long long)ncomp);
    if (scalar_size <= 0) return fail("invalid elem_size");
    if (ncomp > 1 && !(scalar_size == 1 || scalar_size == 2 ||
                       scalar_size == 4 || scalar_size == 8 ||
                       scalar_size == 16))
        return fail("invalid scalar_size %lld for ncomp %lld: must be 1, 2, "
                    "4, 8 or 16", (long long)scalar_size, (long long)ncomp);
    return 0;
}

static pa_status select_kernel_comp(const CopyDescH &dn, int64_t ssz,
                                    int64_t ncomp, const void *src,
                                    const void *dst, KernelSel *out)
{
    if (pa_status cst = check_comp(ssz, ncomp)) return cst;
    /* one scalar per element: exactly the plain elem_size decision */
    if (ncomp == 1) return select_kernel(dn, ssz, src, dst, out);
    const int64_t B = ssz * ncomp;
    /* power-of-two totals (2 x f32, 2 x f64, 4 x f16): the tuned tiles */
    if (B == 1 || B == 2 || B == 4 || B == 8 || B == 16)
        return select_kernel(dn, B, src, dst, out);

    *out = KernelSel();
    if (dn.total == 0) return 0;
    const uintptr_t ptrs = (uintptr_t)src | (uintptr_t)dst;

    if (dn.sstr[0] == 1 && dn.dstr[0] == 1) {
        /* linear at element level: widest word dividing the run, every
         * stride/offset in bytes, and both base addresses */
        CopyDescH w;
        int64_t W = 0;
        for (int64_t cand : {16, 8, 4, 2, 1})
            if ((ptrs & (uintptr_t)(cand - 1)) == 0 &&
                word_scale(dn, B, cand, &w)) { W = cand; break; }
        if (!W) return fail("word_scale(1)");
        out->word = (int)W;
        out->d = w;
        if (w.nd == 1)
            out->kind = (W == 16 && w.total * 16 >= (512ll << 20))
                            ? PA_KERNEL_COPY_1D_NT
                            : PA_KERNEL_COPY_1D;
        else
            out->kind = PA_KERNEL_LINEAR;
        return 0;
    }

    /* every offset and stride is a whole number of elements, so only the
     * base pointers can lower the word below the largest power of two
     * dividing B */
    int64_t W = 16;
    while (W > 1 && (B % W || (ptrs & (uintptr_t)(W - 1)))) W >>= 1;
    const int64_t m = B / W;

    int ta = -1;
    if (dn.sstr[0] == 1)
        for (int a = 1; a < dn.nd; a++)
            if (dn.dstr[a] == 1) { ta = a; break; }

    if (ta > 0 && B <= PA_WIDE_MAX_BYTES) {
        out->kind = PA_KERNEL_TILE_WIDE;
        out->word = (int)W;
        out->m = (int)m;
        out->ta = ta;
        out->d = dn;
        wide_tile_shape(B, &out->ti, &out->tj);
        /* LDS row pitch in words: >= ti*m and == m modulo the 256-B bank
         * span, so the store phase's m-word runs land on consecutive
         * banks across the row jump */
        const int64_t span = 256 / W;
        out->pitch =
            (int)(m + ((int64_t)(out->ti - 1) * m + span - 1) / span * span);
        return 0;
    }

    /* no contiguous axis, or an element past the wide-tile cap: expand to
     * words (an inner axis of m unit-stride words) and run the linear
     * kernel — correct and slow */
    {
        if (dn.nd + 1 > MAXND) return fail("too many dims to word-expand");
        int64_t dims[MAXND + 1], ss[MAXND + 1], ds[MAXND + 1];
        dims[0] = m;
        ss[0] = 1;
        ds[0] = 1;
        for (int a = 0; a < dn.nd; a++) {
            dims[a + 1] = dn.dims[a];
            ss[a + 1] = dn.sstr[a] * m;
            ds[a + 1] = dn.dstr[a] * m;
        }
        out->d = normalize_desc(dn.nd + 1, dims, ss, dn.soff * m, ds,
                                dn.doff * m);
        if (out->d.sstr[0] != 1 || out->d.dstr[0] != 1)
            return fail("word expansion lost its unit axis");
        out->kind = out->d.nd == 1 ? PA_KERNEL_COPY_1D : PA_KERNEL_LINEAR;
        out->word = (int)W;
        out->m = (int)m;
        return 0;
    }
}

/* ---- runtime values -> template instances ------------------------------
 *
 * Each kernel family has ONE dispatcher that checks the runtime parameters
 * and calls a generic callable with compile-time tags; the single-descriptor
 * launcher and the grouped launcher of a family are the callables, which name
 * their kernel template and its arguments and nothing else. */

template <typename T> struct Tag { typedef T type; };
template <int I> using Int = std::integral_constant<int, I>;

/* a kernel launch as an expression, for the dispatchers' callables */
template <typename K, typename... A>
static pa_status launch(K kern, dim3 grid, dim3 block, size_t lds,
                        hipStream_t stream, const A &...args)
{
    hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
    return 0;
}

/* word bytes -> f(Tag<word type>) */
template <typename F> static pa_status for_word(int W, F &&f)
{
    switch (W) {
    case 16: return f(Tag<uint4>{});
    case 8: return f(Tag<uint64_t>{});
    case 4: return f(Tag<uint32_t>{});
    case 2: return f(Tag<uint16_t>{});
    case 1: return f(Tag<uint8_t>{});
    default: return fail("bad word width %d", W);
    }
}

/* sweep depth -> f(Int<JCHUNK>), the depths sweep_depth() hands out */
template <typename F> static pa_status for_sweep(int sweep, F &&f)
{
    return sweep == 32 ? f(Int<32>{}) : sweep == 8 ? f(Int<8>{}) : f(Int<1>{});
}

/* scalars per access of a linear kernel -> f(Int<V>): the powers of two up
 * to VMAX = 16 / (widest scalar), so V == 4 exists only where that scalar
 * has 4 bytes */
template <int VMAX, typename F> static pa_status for_vec(int V, F &&f)
{
    if constexpr (VMAX >= 4)
        if (V == 4) return f(Int<4>{});
    if constexpr (VMAX >= 2)
        if (V == 2) return f(Int<2>{});
    if (V == 1) return f(Int<1>{});
    return fail("bad vector width %d", V);
}

/* scalars per element of a tile kernel -> f(Int<N>), N in LO..4 */
template <int LO, typename F> static pa_status for_count(int n, F &&f)
{
    switch (n) {
    case 1:
        if constexpr (LO <= 1) return f(Int<1>{});
        break;
    case 2: return f(Int<2>{});
    case 3: return f(Int<3>{});
    case 4: return f(Int<4>{});
    }
    return fail("bad component count %d", n);
}

/* workgroups of one launch, and the tile counts the tile kernels take */
struct Grid {
    int64_t nti = 0, njc = 0, nblocks = 0;
};

/* the grid of a copy selection: what launch_sel() launches and what a stage
 * table adds up */
static Grid sel_grid(const KernelSel &k)
{
    const CopyDescH &w = k.d;
    Grid g;
    int ti = 0, tj = 0;
    switch (k.kind) {
    case PA_KERNEL_NONE:
        return g;
    case PA_KERNEL_COPY_1D:
    case PA_KERNEL_COPY_1D_NT:
    case PA_KERNEL_LINEAR:
        g.nblocks = grid_exact(w.total, 256);
        return g;
    case PA_KERNEL_GENERIC:
        g.nblocks = grid_for(w.total, 256);
        return g;
    case PA_KERNEL_TILE:
        ti = k.word == 16 ? 32 : 128;
        tj = k.word == 16 ? 32 : 64;
        break;
    case PA_KERNEL_TILE_VS:
        ti = 64;
        tj = 128;
        break;
    case PA_KERNEL_TILE_PK:
        ti = tj = 128;
        break;
    default: /* PA_KERNEL_TILE_WIDE */
        ti = k.ti;
        tj = k.tj;
        break;
    }
    int64_t nbatch = 1;
    for (int a = 1; a < w.nd; a++)
        if (a != k.ta) nbatch *= w.dims[a];
    const int64_t ntj = (w.dims[k.ta] + tj - 1) / tj;
    g.nti = (w.dims[0] + ti - 1) / ti;
    g.njc = (ntj + k.sweep - 1) / k.sweep;
    g.nblocks = g.nti * g.njc * nbatch;
    return g;
}

static pa_status launch_sel(const KernelSel &k, const void *src, void *dst,
                            hipStream_t stream)
{
    if (k.kind == PA_KERNEL_NONE) return 0;
    const CopyDescH &w = k.d;
    const Grid g = sel_grid(k);
    const int ta = k.ta;
    pa_status st = for_word(k.word, [&](auto tag) -> pa_status {
        using T = typename decltype(tag)::type;
        const T *s = (const T *)src;
        T *d = (T *)dst;
        dim3 grid;
        switch (k.kind) {
        case PA_KERNEL_COPY_1D:
            if (pa_status gst = grid2d(g.nblocks, 256, &grid)) return gst;
            return launch(k_copy_1d<T>, grid, dim3(256), 0, stream,
                          s + w.soff, d + w.doff, w.total);
        case PA_KERNEL_COPY_1D_NT:
            if constexpr (sizeof(T) == 16) {
                if (pa_status gst = grid2d(g.nblocks, 256, &grid)) return gst;
                return launch(k_copy_1d_nt, grid, dim3(256), 0, stream,
                              s + w.soff, d + w.doff, w.total);
            }
            break;
        case PA_KERNEL_LINEAR:
            if (pa_status gst = grid2d(g.nblocks, 256, &grid)) return gst;
            return launch(k_copy_linear<T>, grid, dim3(256), 0, stream, s, d,
                          to_dev(w));
        case PA_KERNEL_GENERIC: /* grid-stride kernel */
            return launch(k_copy_generic<T>, dim3((uint32_t)g.nblocks),
                          dim3(256), 0, stream, s, d, to_dev(w));
        case PA_KERNEL_TILE:
            /* 16-byte words: 32x32; 4- and 8-byte: 128x64 with a sweep;
             * 1- and 2-byte: 128x64, one tile per workgroup */
            if constexpr (sizeof(T) == 16) {
                if (pa_status gst = grid2d(g.nblocks, 64 * 8, &grid))
                    return gst;
                return launch(k_transpose_tile<T, 32, 32, 8, 1>, grid,
                              dim3(64, 8), 0, stream, s, d, to_dev(w), ta,
                              g.nti, g.njc, g.nblocks);
            } else {
                if (pa_status gst = grid2d(g.nblocks, 64 * 16, &grid))
                    return gst;
                if constexpr (sizeof(T) >= 4)
                    return for_sweep(k.sweep, [&](auto jc) {
                        return launch(
                            k_transpose_tile<T, 128, 64, 16,
                                             decltype(jc)::value>,
                            grid, dim3(64, 16), 0, stream, s, d, to_dev(w),
                            ta, g.nti, g.njc, g.nblocks);
                    });
                else
                    return launch(k_transpose_tile<T, 128, 64, 16, 1>, grid,
                                  dim3(64, 16), 0, stream, s, d, to_dev(w),
                                  ta, g.nti, g.njc, g.nblocks);
            }
        case PA_KERNEL_TILE_VS:
            if constexpr (sizeof(T) == 8) {
                if (pa_status gst = grid2d(g.nblocks, 64 * 16, &grid))
                    return gst;
                return for_sweep(k.sweep, [&](auto jc) {
                    constexpr int JC = decltype(jc)::value;
                    return launch(
                        k.stream ? k_transpose_tile_vs_nt<T, 64, 128, 16, JC>
                                 : k_transpose_tile_vs<T, 64, 128, 16, JC>,
                        grid, dim3(64, 16), 0, stream, s, d, to_dev(w), ta,
                        g.nti, g.njc, g.nblocks);
                });
            }
            break;
        case PA_KERNEL_TILE_PK:
            if constexpr (sizeof(T) <= 2) {
                if (pa_status gst = grid2d(g.nblocks, 256, &grid)) return gst;
                return launch(k_transpose_tile_pk<T, 128, 128, 256>, grid,
                              dim3(256), 0, stream, s, d, to_dev(w), ta,
                              g.nti, g.njc, g.nblocks);
            }
            break;
        case PA_KERNEL_TILE_WIDE: {
            if (k.m < 2 || k.ti < 1 || k.tj < 1 || k.pitch < k.ti * k.m)
                return fail("bad wide-tile selection");
            if (pa_status gst = grid2d(g.nblocks, 256, &grid)) return gst;
            const size_t lds = (size_t)k.tj * k.pitch * sizeof(T);
            if (lds > (64u << 10))
                return fail("wide tile needs %zu B of LDS", lds);
            const uint32_t magic =
                (uint32_t)((((uint64_t)1 << 32) + k.m - 1) / k.m);
            return launch(k.m == 3 ? k_transpose_tile_wide<T, 3>
                                   : k_transpose_tile_wide<T, 0>,
                          grid, dim3(64, 4), lds, stream, s, d, to_dev(w), ta,
                          k.m, magic, k.ti, k.tj, k.pitch, g.nti, g.njc,
                          g.nblocks);
        }
        default:
            return fail("bad kernel kind %d", k.kind);
        }
        return fail("kernel kind %d has no %d-byte word", k.kind, k.word);
    });
    if (st) return st;
    HIP_CHECK(hipGetLastError());
    return 0;
}

static pa_status launch_desc(const CopyDescH &dn, int64_t ssz, int64_t ncomp,
                             const void *src, void *dst, hipStream_t stream)
{
    KernelSel k;
    pa_status st = select_kernel_comp(dn, ssz, ncomp, src, dst, &k);
    if (st) return st;
    return launch_sel(k, src, dst, stream);
}

/* ---- reduced-precision wire: selection and launch ---------------------- */

/* The decision for a converting copy, made in ONE place like select_kernel():
 * launch_cvt_sel() executes it, pa_copy_kernel_kind_wire() reports it. */
struct CvtSel {
    int kind = PA_KERNEL_NONE;
    int wire = 0, op = 0, ncomp = 1;
    int scalar = 0;     /* PA_KERNEL_SCALE_*: PA_SCALAR_*, wire = op = 0 */
    int V = 1;          /* scalars per access (linear) */
    int ti = 0, tj = 0; /* tile shape in elements (tile) */
    int ta = -1;        /* dst-contiguous axis (tile) */
    CopyDescH d;        /* linear: in units of V scalars; else elements */
};

#define PA_CVT_TILE_MAX_COMP 4

/* stored / wire scalar bytes of a wire pair; false for an unknown code */
static bool wire_sizes(int wire, int64_t *stored, int64_t *wsz)
{
    switch (wire) {
    case PA_WIRE_F64_F32: *stored = 8; *wsz = 4; return true;
    case PA_WIRE_F32_F16:
    case PA_WIRE_F32_BF16: *stored = 4; *wsz = 2; return true;
    default: return false;
    }
}

static pa_status check_wire(int wire, int op, int64_t ncomp)
{
    int64_t a, b;
    if (!wire_sizes(wire, &a, &b)) return fail("unknown wire pair %d", wire);
    if (op != PA_WIRE_NARROW && op != PA_WIRE_WIDEN && op != PA_WIRE_ROUND)
        return fail("unknown wire op %d", op);
    if (ncomp < 1) return fail("invalid ncomp %lld", (long long)ncomp);
    return 0;
}

/* The linear / tile / generic decision shared by the converting and the
 * scaling selectors, for elements of ncomp scalars of ssz bytes at the source
 * and dsz bytes at the destination.  Linear: the components join the
 * contiguous axis and out->d is in units of out->V scalars.  Tile: out->ta is
 * the destination-contiguous axis; the caller sets the tile shape. */
enum { SHAPE_LINEAR, SHAPE_TILE, SHAPE_GENERIC };

static int select_shape(const CopyDescH &dn, int64_t ssz, int64_t dsz,
                        int64_t ncomp, const void *src, const void *dst,
                        CvtSel *out)
{
    if (dn.sstr[0] == 1 && dn.dstr[0] == 1) {
        /* scalar units: the components join the contiguous axis */
        CopyDescH w = dn;
        w.dims[0] *= ncomp;
        w.soff *= ncomp;
        w.doff *= ncomp;
        for (int a = 1; a < w.nd; a++) {
            w.sstr[a] *= ncomp;
            w.dstr[a] *= ncomp;
        }
        /* V scalars per access, each access naturally aligned on both
         * sides: V divides the run, both offsets, every non-unit stride and
         * (in scalars) both base addresses */
        int64_t V = 16 / std::max(ssz, dsz);
        auto ok = [&](int64_t v) {
            if (w.dims[0] % v || w.soff % v || w.doff % v) return false;
            if ((uintptr_t)src % (uintptr_t)(v * ssz)) return false;
            if ((uintptr_t)dst % (uintptr_t)(v * dsz)) return false;
            for (int a = 1; a < w.nd; a++)
                if (w.sstr[a] % v || w.dstr[a] % v) return false;
            return true;
        };
        while (V > 1 && !ok(V)) V >>= 1;
        w.dims[0] /= V;
        w.soff /= V;
        w.doff /= V;
        for (int a = 1; a < w.nd; a++) {
            w.sstr[a] /= V;
            w.dstr[a] /= V;
        }
        w.total = 1;
        for (int a = 0; a < w.nd; a++) w.total *= w.dims[a];
        out->V = (int)V;
        out->d = w;
        return SHAPE_LINEAR;
    }

    out->d = dn;
    int ta = -1;
    if (dn.sstr[0] == 1)
        for (int a = 1; a < dn.nd; a++)
            if (dn.dstr[a] == 1) { ta = a; break; }
    if (ta > 0 && ncomp <= PA_CVT_TILE_MAX_COMP) {
        out->ta = ta;
        return SHAPE_TILE;
    }
    return SHAPE_GENERIC;
}

static pa_status select_kernel_cvt(const CopyDescH &dn, int wire, int op,
                                   int64_t ncomp, const void *src,
                                   const void *dst, CvtSel *out)
{
    if (pa_status st = check_wire(wire, op, ncomp)) return st;
    *out = CvtSel();
    out->wire = wire;
    out->op = op;
    out->ncomp = (int)ncomp;
    if (dn.total == 0) return 0;
    int64_t stored, wsz;
    wire_sizes(wire, &stored, &wsz);
    const int64_t ssz = op == PA_WIRE_WIDEN ? wsz : stored;
    const int64_t dsz = op == PA_WIRE_NARROW ? wsz : stored;
    switch (select_shape(dn, ssz, dsz, ncomp, src, dst, out)) {
    case SHAPE_LINEAR:
        out->kind = PA_KERNEL_CVT_LINEAR;
        break;
    case SHAPE_TILE:
        out->kind = PA_KERNEL_CVT_TILE;
        out->ti = cvt_tile_ti((int)ncomp);
        out->tj = CVT_TILE_TJ;
        break;
    default:
        out->kind = PA_KERNEL_CVT_GENERIC;
    }
    return 0;
}

/* workgroups of a converting or scaling selection: the grid launch_cvt_sel()
 * resp. launch_scale_sel() launches */
static int64_t cvt_grid(const CvtSel &k, int64_t *nti, int64_t *ntj)
{
    const CopyDescH &w = k.d;
    *nti = *ntj = 0;
    switch (k.kind) {
    case PA_KERNEL_CVT_LINEAR:
    case PA_KERNEL_SCALE_LINEAR:
        return grid_exact(w.total, 256);
    case PA_KERNEL_CVT_GENERIC:
    case PA_KERNEL_SCALE_GENERIC:
        return grid_for(w.total * k.ncomp, 256);
    case PA_KERNEL_CVT_TILE:
    case PA_KERNEL_SCALE_TILE: {
        int64_t nbatch = 1;
        for (int a = 1; a < w.nd; a++)
            if (a != k.ta) nbatch *= w.dims[a];
        *nti = (w.dims[0] + k.ti - 1) / k.ti;
        *ntj = (w.dims[k.ta] + k.tj - 1) / k.tj;
        return *nti * *ntj * nbatch;
    }
    default:
        return 0;
    }
}

/* the launch grid of a converting or scaling kind over nblocks workgroups:
 * 256 threads (linear), 64 x 16 (tile), a 1-D grid-stride grid (generic) */
static pa_status cvt_dim(int kind, int64_t nblocks, dim3 *grid)
{
    switch (kind) {
    case PA_KERNEL_CVT_LINEAR:
    case PA_KERNEL_SCALE_LINEAR:
        return grid2d(nblocks, 256, grid);
    case PA_KERNEL_CVT_TILE:
    case PA_KERNEL_SCALE_TILE:
        return grid2d(nblocks, 64 * 16, grid);
    default:
        *grid = dim3((uint32_t)nblocks);
        return 0;
    }
}

/* The converting family: (wire, op), then V (linear) or the component count
 * (tile), become lin(Int<WIRE>, Int<OP>, Int<V>), tile(Int<WIRE>, Int<OP>,
 * Int<NC>) or gen(Int<WIRE>, Int<OP>). */
template <typename L, typename T, typename G>
static pa_status for_cvt(const CvtSel &k, L &&lin, T &&tile, G &&gen)
{
    auto shape = [&](auto w, auto o) -> pa_status {
        /* the widest scalar of the pair is the stored one */
        constexpr int VMAX = decltype(w)::value == PA_WIRE_F64_F32 ? 2 : 4;
        switch (k.kind) {
        case PA_KERNEL_CVT_LINEAR:
            return for_vec<VMAX>(k.V, [&](auto v) { return lin(w, o, v); });
        case PA_KERNEL_CVT_TILE:
            return for_count<1>(k.ncomp,
                                [&](auto nc) { return tile(w, o, nc); });
        case PA_KERNEL_CVT_GENERIC:
            return gen(w, o);
        default:
            return fail("bad converting kernel kind %d", k.kind);
        }
    };
    switch (k.wire * 3 + k.op) {
    case 3: return shape(Int<1>{}, Int<0>{});
    case 4: return shape(Int<1>{}, Int<1>{});
    case 5: return shape(Int<1>{}, Int<2>{});
    case 6: return shape(Int<2>{}, Int<0>{});
    case 7: return shape(Int<2>{}, Int<1>{});
    case 8: return shape(Int<2>{}, Int<2>{});
    case 9: return shape(Int<3>{}, Int<0>{});
    case 10: return shape(Int<3>{}, Int<1>{});
    case 11: return shape(Int<3>{}, Int<2>{});
    default: return fail("bad wire pair %d / op %d", k.wire, k.op);
    }
}

static pa_status launch_cvt_sel(const CvtSel &k, const void *src, void *dst,
                                hipStream_t stream)
{
    if (k.kind == PA_KERNEL_NONE) return 0;
    /* the tile shape the kernel assumes; checked here because it does not
     * depend on the instance (the scaling tile's does: see its tile lambda) */
    if (k.kind == PA_KERNEL_CVT_TILE &&
        (k.ta < 1 || k.ti != cvt_tile_ti(k.ncomp) || k.tj != CVT_TILE_TJ))
        return fail("bad converting-tile selection");
    int64_t nti, ntj;
    const int64_t nblocks = cvt_grid(k, &nti, &ntj);
    const DescDev dd = to_dev(k.d);
    dim3 grid;
    if (pa_status gst = cvt_dim(k.kind, nblocks, &grid)) return gst;
    pa_status st = for_cvt(
        k,
        [&](auto w, auto o, auto v) {
            return launch(k_cvt_linear<w, o, v>, grid, dim3(256), 0, stream,
                          src, dst, dd);
        },
        [&](auto w, auto o, auto nc) {
            return launch(k_cvt_tile<w, o, nc>, grid, dim3(64, 16), 0, stream,
                          src, dst, dd, k.ta, nti, ntj, nblocks);
        },
        [&](auto w, auto o) {
            return launch(k_cvt_generic<w, o>, grid, dim3(256), 0, stream,
                          src, dst, dd, k.ncomp);
        });
    if (st) return st;
    HIP_CHECK(hipGetLastError());
    return 0;
}

static pa_status launch_desc_cvt(const CopyDescH &dn, int wire, int op,
                                 int64_t ncomp, const void *src, void *dst,
                                 hipStream_t stream)
{
    CvtSel k;
    pa_status st = select_kernel_cvt(dn, wire, op, ncomp, src, dst, &k);
    if (st) return st;
    return launch_cvt_sel(k, src, dst, stream);
}

/* ---- scaled copies: selection and launch ------------------------------ */

/* bytes of a PA_SCALAR_* code, 0 for an unknown one */
static int64_t scalar_bytes(int scalar)
{
    return scalar == PA_SCALAR_F32 ? 4 : scalar == PA_SCALAR_F64 ? 8 : 0;
}

static pa_status check_scale(int scalar, int64_t nscal, double alpha)
{
    if (!scalar_bytes(scalar))
        return fail("unknown scalar type %d (PA_SCALAR_F32 = 1, "
                    "PA_SCALAR_F64 = 2)", scalar);
    if (nscal < 1) return fail("invalid nscal %lld", (long long)nscal);
    if (!std::isfinite(alpha)) return fail("scale alpha must be finite");
    return 0;
}

/* The decision for a scaling copy, in ONE place: launch_scale_sel() executes
 * it, pa_copy_kernel_kind_scale() reports it.  The rules are those of
 * select_kernel_cvt() with one scalar type on both sides; the selection
 * lives in a CvtSel (ncomp = scalars per element). */
static pa_status select_kernel_scale(const CopyDescH &dn, int scalar,
                                     int64_t nscal, const void *src,
                                     const void *dst, CvtSel *out)
{
    if (pa_status st = check_scale(scalar, nscal, 0.0)) return st;
    *out = CvtSel();
    out->scalar = scalar;
    out->ncomp = (int)nscal;
    if (dn.total == 0) return 0;
    const int64_t sz = scalar_bytes(scalar);
    switch (select_shape(dn, sz, sz, nscal, src, dst, out)) {
    case SHAPE_LINEAR:
        out->kind = PA_KERNEL_SCALE_LINEAR;
        break;
    case SHAPE_TILE:
        out->kind = PA_KERNEL_SCALE_TILE;
        out->ti = scalar == PA_SCALAR_F32 ? scale_tile_ti<float>((int)nscal)
                                          : scale_tile_ti<double>((int)nscal);
        out->tj = SCALE_TILE_TJ;
        break;
    default:
        out->kind = PA_KERNEL_SCALE_GENERIC;
    }
    return 0;
}

/* The scaling family: the scalar type, then V (linear) or the scalars per
 * element (tile), become lin(a, Int<V>), tile(a, Int<NC>) or gen(a), with
 * a = S(alpha) carrying the scalar type S. */
template <typename L, typename T, typename G>
static pa_status for_scale(const CvtSel &k, double alpha, L &&lin, T &&tile,
                           G &&gen)
{
    auto shape = [&](auto a) -> pa_status {
        constexpr int VMAX = 16 / (int)sizeof(a);
        switch (k.kind) {
        case PA_KERNEL_SCALE_LINEAR:
            return for_vec<VMAX>(k.V, [&](auto v) { return lin(a, v); });
        case PA_KERNEL_SCALE_TILE:
            return for_count<1>(k.ncomp, [&](auto nc) { return tile(a, nc); });
        case PA_KERNEL_SCALE_GENERIC:
            return gen(a);
        default:
            return fail("bad scaling kernel kind %d", k.kind);
        }
    };
    if (k.scalar == PA_SCALAR_F32) return shape((float)alpha);
    if (k.scalar == PA_SCALAR_F64) return shape(alpha);
    return fail("bad scalar type %d", k.scalar);
}

static pa_status launch_scale_sel(const CvtSel &k, const void *src, void *dst,
                                  double alpha, hipStream_t stream)
{
    if (k.kind == PA_KERNEL_NONE) return 0;
    int64_t nti, ntj;
    const int64_t nblocks = cvt_grid(k, &nti, &ntj);
    const DescDev dd = to_dev(k.d);
    dim3 grid;
    if (pa_status gst = cvt_dim(k.kind, nblocks, &grid)) return gst;
    pa_status st = for_scale(
        k, alpha,
        [&](auto a, auto v) {
            return launch(k_scale_linear<decltype(a), v>, grid, dim3(256), 0,
                          stream, src, dst, dd, a);
        },
        [&](auto a, auto nc) -> pa_status {
            /* the tile shape the kernel assumes depends on the scalar type,
             * so the check sits where that type is known */
            if (k.ta < 1 || k.ti != scale_tile_ti<decltype(a)>(k.ncomp) ||
                k.tj != SCALE_TILE_TJ)
                return fail("bad scaling-tile selection");
            return launch(k_scale_tile<decltype(a), nc>, grid, dim3(64, 16),
                          0, stream, src, dst, dd, k.ta, nti, ntj, nblocks, a);
        },
        [&](auto a) {
            return launch(k_scale_generic<decltype(a)>, grid, dim3(256), 0,
                          stream, src, dst, dd, k.ncomp, a);
        });
    if (st) return st;
    HIP_CHECK(hipGetLastError());
    return 0;
}

/* ---- split / join copies: selection and launch ------------------------ */

/* The decision for a split or join copy, made in ONE place like
 * select_kernel(): launch_soa_sel() executes it, pa_copy_kernel_kind_soa()
 * reports it. */
struct SoaSel {
    int kind = PA_KERNEL_NONE;
    int ssz = 0, n = 0, dir = 0;
    int V = 1;          /* scalars per access (linear) */
    int ti = 0, tj = 0; /* tile shape in elements (tile) */
    int pitch = 0, plane = 0; /* LDS row pitch and component plane, words */
    int ta = -1;        /* dst-contiguous axis (tile) */
    CopyDescH d;        /* linear: in units of V scalars; else scalars */
};

static pa_status check_soa(int64_t scalar_size, int n, int dir)
{
    if (n < 2) return fail("n must be >= 2 (got %d)", n);
    if (scalar_size != 4 && scalar_size != 8 && scalar_size != 16)
        return fail("invalid scalar_size %lld for a split or join: must be "
                    "4, 8 or 16", (long long)scalar_size);
    if (dir != PA_SOA_SPLIT && dir != PA_SOA_JOIN)
        return fail("unknown direction %d: PA_SOA_SPLIT or PA_SOA_JOIN", dir);
    return 0;
}

static pa_status select_kernel_soa(const CopyDescH &dn, int64_t ssz, int n,
                                   int dir, const void *aos,
                                   const void *const *fields, SoaSel *out)
{
    if (pa_status st = check_soa(ssz, n, dir)) return st;
    *out = SoaSel();
    out->ssz = (int)ssz;
    out->n = n;
    out->dir = dir;
    if (dn.total == 0) return 0;
    out->d = dn;
    /* every kernel accesses whole scalars (a 16-byte one as uint4) */
    if ((uintptr_t)aos % (uintptr_t)ssz)
        return fail("the vector-valued array pointer is not aligned to the "
                    "%lld-byte scalar", (long long)ssz);
    for (int c = 0; fields && c < n; c++)
        if ((uintptr_t)fields[c] % (uintptr_t)ssz)
            return fail("the pointer of field %d is not aligned to the "
                        "%lld-byte scalar", c, (long long)ssz);
    const bool small = n <= PA_SOA_TILE_MAX_N &&
                       (int64_t)n * ssz <= PA_WIDE_MAX_BYTES;

    if (small && dn.sstr[0] == 1 && dn.dstr[0] == 1) {
        /* V scalars per access, each access naturally aligned on both
         * sides: V divides the run, both offsets, every non-unit stride and
         * (in scalars) the AoS base and every field base.  The AoS offset
         * n * (element offset) follows the element offset. */
        uintptr_t ptrs = (uintptr_t)aos;
        for (int c = 0; c < n; c++) ptrs |= (uintptr_t)(fields ? fields[c] : 0);
        CopyDescH w = dn;
        int64_t V = 16 / ssz;
        auto ok = [&](int64_t v) {
            if (w.dims[0] % v || w.soff % v || w.doff % v) return false;
            if (ptrs % (uintptr_t)(v * ssz)) return false;
            for (int a = 1; a < w.nd; a++)
                if (w.sstr[a] % v || w.dstr[a] % v) return false;
            return true;
        };
        while (V > 1 && !ok(V)) V >>= 1;
        w.dims[0] /= V;
        w.soff /= V;
        w.doff /= V;
        for (int a = 1; a < w.nd; a++) {
            w.sstr[a] /= V;
            w.dstr[a] /= V;
        }
        w.total = 1;
        for (int a = 0; a < w.nd; a++) w.total *= w.dims[a];
        out->kind = PA_KERNEL_SOA_LINEAR;
        out->V = (int)V;
        out->d = w;
        return 0;
    }

    int ta = -1;
    if (dn.sstr[0] == 1)
        for (int a = 1; a < dn.nd; a++)
            if (dn.dstr[a] == 1) { ta = a; break; }
    if (small && ta > 0) {
        out->kind = PA_KERNEL_SOA_TILE;
        out->ta = ta;
        wide_tile_shape(n * ssz, &out->ti, &out->tj);
        /* LDS pitch == n modulo the 256-B bank span (in words), and for a
         * join's planar tile plane == 1: see k_soa_tile */
        const int64_t span = 256 / ssz;
        const int64_t row = dir == PA_SOA_SPLIT ? (int64_t)out->ti * n : out->ti;
        out->pitch = (int)(n + (row - n + span - 1) / span * span);
        if (dir == PA_SOA_JOIN)
            out->plane = (int)(1 + ((int64_t)out->tj * out->pitch - 1 +
                                    span - 1) / span * span);
        return 0;
    }
    out->kind = PA_KERNEL_SOA_GENERIC;
    return 0;
}

/* workgroups per component of the grid-stride generic split / join kernel */
static int soa_generic_gx(const SoaSel &k)
{
    return grid_for(k.d.total, 256);
}

/* the grid of a split / join selection: what launch_soa_sel() launches and
 * what a stage table adds up.  The generic kernel's count is over all n
 * components (its launches spread them over blockIdx.z). */
static Grid soa_grid(const SoaSel &k)
{
    Grid g;
    switch (k.kind) {
    case PA_KERNEL_SOA_LINEAR:
        g.nblocks = grid_exact(k.d.total, 256);
        break;
    case PA_KERNEL_SOA_GENERIC:
        g.nblocks = (int64_t)soa_generic_gx(k) * k.n;
        break;
    case PA_KERNEL_SOA_TILE: {
        int64_t nbatch = 1;
        for (int a = 1; a < k.d.nd; a++)
            if (a != k.ta) nbatch *= k.d.dims[a];
        g.nti = (k.d.dims[0] + k.ti - 1) / k.ti;
        g.njc = (k.d.dims[k.ta] + k.tj - 1) / k.tj;
        g.nblocks = g.nti * g.njc * nbatch;
        break;
    }
    default:
        break;
    }
    return g;
}

/* the kernel argument holding the multiplier policy and N field pointers,
 * the first nc of them set */
template <int N, typename M>
static SoaPtrs<N, M> soa_ptrs(const M &m, void *const *fields, int nc)
{
    SoaPtrs<N, M> f;
    static_cast<M &>(f) = m;
    for (int c = 0; c < N; c++) f.p[c] = c < nc ? fields[c] : nullptr;
    return f;
}

/* The scalar sizes a scale of real type `scalar` applies to: one scalar or
 * two (a complex scalar), nothing else. */
static pa_status check_soa_scale(int64_t ssz, int scalar, double alpha)
{
    if (pa_status st = check_scale(scalar, 1, alpha)) return st;
    const int64_t sz = scalar_bytes(scalar);
    if (ssz != sz && ssz != 2 * sz)
        return fail("a %lld-byte scalar is neither one nor two of the "
                    "%lld-byte real scalars of the scale",
                    (long long)ssz, (long long)sz);
    return 0;
}

/* The split / join family: the scalar word S, the multiplier policy, the
 * direction and N, then V (linear) or the tile's LDS bytes, become
 * lin(Tag<S>, m, Int<DIR>, Int<N>, Int<V>), tile(Tag<S>, m, Int<DIR>, Int<N>,
 * lds) or gen(Tag<S>, m, Int<DIR>).  m is the policy value: SoaNoMul for a
 * plain call (scalar == 0), SoaMul<R> holding R(alpha) for a scaled one, S
 * being one or two R. */
template <typename L, typename T, typename G>
static pa_status for_soa(const SoaSel &k, int scalar, double alpha, L &&lin,
                         T &&tile, G &&gen)
{
    if (scalar)
        if (pa_status st = check_soa_scale(k.ssz, scalar, alpha)) return st;
    auto shape = [&](auto s, auto m, auto dir) -> pa_status {
        using S = typename decltype(s)::type;
        if (k.kind == PA_KERNEL_SOA_GENERIC) return gen(s, m, dir);
        if (k.kind != PA_KERNEL_SOA_LINEAR && k.kind != PA_KERNEL_SOA_TILE)
            return fail("bad split/join kernel kind %d", k.kind);
        return for_count<2>(k.n, [&](auto n) -> pa_status {
            if (k.kind == PA_KERNEL_SOA_LINEAR)
                return for_vec<16 / (int)sizeof(S)>(
                    k.V, [&](auto v) { return lin(s, m, dir, n, v); });
            constexpr int N = decltype(n)::value;
            constexpr bool split = decltype(dir)::value == PA_SOA_SPLIT;
            const int64_t row = split ? (int64_t)k.ti * N : k.ti;
            if (k.ta < 1 || k.ti < 1 || k.tj != PA_SOA_TILE_TJ ||
                k.pitch < row || (!split && k.plane < k.tj * k.pitch))
                return fail("bad split/join tile selection");
            const size_t lds = sizeof(S) * (split ? (size_t)k.tj * k.pitch
                                                  : (size_t)N * k.plane);
            if (lds > (64u << 10))
                return fail("split/join tile needs %zu B of LDS", lds);
            return tile(s, m, dir, n, lds);
        });
    };
    auto policy = [&](auto s, auto m) -> pa_status {
        return k.dir == PA_SOA_SPLIT ? shape(s, m, Int<PA_SOA_SPLIT>{})
                                     : shape(s, m, Int<PA_SOA_JOIN>{});
    };
    const SoaNoMul none;
    const SoaMul<float> mf{(float)alpha};
    const SoaMul<double> md{alpha};
    switch (k.ssz) {
    case 4:
        return scalar ? policy(Tag<uint32_t>{}, mf)
                      : policy(Tag<uint32_t>{}, none);
    case 8:
        return scalar == PA_SCALAR_F32   ? policy(Tag<uint64_t>{}, mf)
               : scalar == PA_SCALAR_F64 ? policy(Tag<uint64_t>{}, md)
                                         : policy(Tag<uint64_t>{}, none);
    case 16:
        return scalar ? policy(Tag<uint4>{}, md) : policy(Tag<uint4>{}, none);
    default:
        return fail("bad scalar size %d", k.ssz);
    }
}

/* aos is the source of a split and the destination of a join; scalar is the
 * PA_SCALAR_* code of a scaling launch by alpha, or 0 for a plain one */
static pa_status launch_soa_sel(const SoaSel &k, void *aos,
                                void *const *fields, int scalar, double alpha,
                                hipStream_t stream)
{
    if (k.kind == PA_KERNEL_NONE) return 0;
    const Grid g = soa_grid(k);
    const DescDev dd = to_dev(k.d);
    dim3 grid;
    if (k.kind != PA_KERNEL_SOA_GENERIC)
        if (pa_status gst = grid2d(g.nblocks, 256, &grid)) return gst;
    pa_status st = for_soa(
        k, scalar, alpha,
        [&](auto s, auto m, auto dir, auto n, auto v) {
            using S = typename decltype(s)::type;
            return launch(k_soa_linear<S, dir, n, v, decltype(m)>, grid,
                          dim3(256), 0, stream, aos,
                          soa_ptrs<n>(m, fields, n), dd);
        },
        [&](auto s, auto m, auto dir, auto n, size_t lds) {
            using S = typename decltype(s)::type;
            return launch(k_soa_tile<S, dir, n, decltype(m)>, grid,
                          dim3(64, 4), lds, stream, aos,
                          soa_ptrs<n>(m, fields, n), dd, k.ta, k.ti, k.pitch,
                          k.plane, g.nti, g.njc, g.nblocks);
        },
        [&](auto s, auto m, auto dir) {
            /* grid-stride kernel, at most PA_SOA_GENERIC_PTRS fields a
             * launch, the component on blockIdx.z */
            using S = typename decltype(s)::type;
            const int gx = soa_generic_gx(k);
            for (int c0 = 0; c0 < k.n; c0 += PA_SOA_GENERIC_PTRS) {
                const int nc = std::min(k.n - c0, PA_SOA_GENERIC_PTRS);
                launch(k_soa_generic<S, dir, decltype(m)>, dim3(gx, 1, nc),
                       dim3(256), 0, stream, aos,
                       soa_ptrs<PA_SOA_GENERIC_PTRS>(m, fields + c0, nc), dd,
                       k.n, c0);
            }
            return (pa_status)0;
        });
    if (st) return st;
    HIP_CHECK(hipGetLastError());
    return 0;
}

static pa_status launch_desc_soa(const CopyDescH &dn, int64_t ssz, int n,
                                 int dir, void *aos, void *const *fields,
                                 hipStream_t stream, int scalar = 0,
                                 double alpha = 1.0)
{
    SoaSel k;
    if (pa_status st = select_kernel_soa(dn, ssz, n, dir, aos, fields, &k))
        return st;
    return launch_soa_sel(k, aos, fields, scalar, alpha, stream);
}

/* ---- zero fill: descriptor, store width, launch ----------------------- */

struct FillDescH {
    int nd = 0;
    int64_t dims[MAXND] = {0}, dstr[MAXND] = {0};
    int64_t doff = 0, total = 0;
};

/* drop unit axes, sort by ascending stride, merge contiguous axes */
static FillDescH normalize_fill(int nd, const int64_t *dims,
                                const int64_t *dstr, int64_t doff)
{
    struct Axis { int64_t dim, ds; };
    std::vector<Axis> ax;
    for (int i = 0; i < nd; i++)
        if (dims[i] != 1) ax.push_back({dims[i], dstr[i]});
    if (ax.empty()) ax.push_back({1, 1});
    std::stable_sort(ax.begin(), ax.end(),
                     [](const Axis &a, const Axis &b) { return a.ds < b.ds; });
    std::vector<Axis> m{ax[0]};
    for (size_t i = 1; i < ax.size(); i++) {
        Axis &p = m.back();
        if (ax[i].ds == p.ds * p.dim)
            p.dim *= ax[i].dim;
        else
            m.push_back(ax[i]);
    }
    FillDescH out;
    out.nd = (int)m.size();
    out.total = 1;
    for (int i = 0; i < out.nd; i++) {
        out.dims[i] = m[i].dim;
        out.dstr[i] = m[i].ds;
        out.total *= m[i].dim;
    }
    out.doff = doff;
    return out;
}

/* The fill decision, made in ONE place like select_kernel(): the widest
 * store of 16, 8 or 4 bytes that divides the base pointer, the offset and
 * every non-unit stride in bytes, and the run length (a contiguous window)
 * or the element (any other window); else single bytes. */
struct FillSel {
    int kind = PA_KERNEL_NONE;
    GFill g;
    int64_t nblocks = 0;
};

static pa_status select_fill(const FillDescH &d, int64_t esz, const void *dst,
                             FillSel *out)
{
    *out = FillSel();
    memset(&out->g, 0, sizeof out->g);
    if (esz <= 0) return fail("bad element size");
    if (d.total == 0) return 0;
    const bool run = d.dstr[0] == 1;
    const int64_t unit = run ? d.dims[0] * esz : esz; /* bytes a word divides */
    int64_t W = 1;
    for (int64_t cand : {16, 8, 4}) {
        bool ok = ((uintptr_t)dst & (uintptr_t)(cand - 1)) == 0 &&
                  unit % cand == 0 && (d.doff * esz) % cand == 0;
        for (int a = run ? 1 : 0; a < d.nd && ok; a++)
            if ((d.dstr[a] * esz) % cand) ok = false;
        if (ok) { W = cand; break; }
    }
    GFill &g = out->g;
    g.nd = d.nd;
    g.width = (int)W;
    g.m = run ? 1 : (int)(esz / W);
    g.total = 1;
    for (int a = 0; a < MAXND; a++) {
        g.dims[a] = a < d.nd ? d.dims[a] : 1;
        g.dstr[a] = a < d.nd ? d.dstr[a] * esz / W : 0;
        g.total *= g.dims[a];
    }
    if (run) {
        g.total = g.total / g.dims[0] * (unit / W);
        g.dims[0] = unit / W;
        g.dstr[0] = 1;
    }
    g.doff = d.doff * esz / W;
    g.dst = (void *)dst;
    out->kind = PA_KERNEL_FILL;
    out->nblocks = grid_exact(g.total, 256);
    return 0;
}

/* ================= metadata ======================================== */

struct Range { int64_t lo, hi; };

struct pa_topology {
    int m;
    std::vector<int64_t> dims;
    int64_t nranks;
};

struct pa_pencil {
    pa_topology topo; /* copied: a pencil owns its grid description */
    int n;
    std::vector<int64_t> size_global;
    std::vector<int32_t> decomp; /* length m */
    std::vector<int32_t> perm;   /* length n; perm[i] = logical dim at mem i */
};

static void split_range(int64_t c, int64_t P, int64_t N, Range *r)
{
    r->lo = (N * c) / P; /* data_ranges.jl:4-9 */
    r->hi = (N * (c + 1)) / P;
}

static void cart_coords(const pa_topology &t, int rank, int64_t *coords)
{
    int64_t rem = rank;
    for (int i = 0; i < t.m; i++) {
        int64_t stride = 1;
        for (int j = i + 1; j < t.m; j++) stride *= t.dims[j];
        coords[i] = rem / stride;
        rem %= stride;
    }
}

static int cart_rank(const pa_topology &t, const int64_t *coords)
{
    int64_t r = 0;
    for (int i = 0; i < t.m; i++) r = r * t.dims[i] + coords[i];
    return (int)r;
}

static void axes_for_coords(const pa_pencil &p, const int64_t *coords,
                            Range *out)
{
    for (int d = 0; d < p.n; d++) {
        out[d].lo = 0;
        out[d].hi = p.size_global[d];
    }
    for (int j = 0; j < p.topo.m; j++)
        split_range(coords[j], p.topo.dims[j], p.size_global[p.decomp[j]],
                    &out[p.decomp[j]]);
}

static void axes_for_rank(const pa_pencil &p, int rank, Range *out)
{
    int64_t coords[MAXND];
    cart_coords(p.topo, rank, coords);
    axes_for_coords(p, coords, out);
}

static void range_intersect(const Range &a, const Range &b, Range *out)
{
    out->lo = std::max(a.lo, b.lo);
    out->hi = std::max(out->lo, std::min(a.hi, b.hi));
}

static int64_t region_nelem(int n, const Range *r)
{
    int64_t v = 1;
    for (int d = 0; d < n; d++) v *= (r[d].hi - r[d].lo);
    return v;
}

/* ================= comm ============================================ */

struct pa_comm {
    ncclComm_t comm;
    int nranks, rank;
};

/* ================= plan ============================================ */

/* one sub-block of a block: its staging block (offset and count in
 * elements) and its descriptor.  Under a keep set a block has one per
 * non-empty sub-box; on an ordinary plan, whose keep set is everything, it
 * has at most one, the block itself. */
struct SubC {
    int64_t off, n;
    CopyDescH d;
};

struct PeerBlockC {
    int k, grank;
    int64_t send_off = 0, recv_off = 0, send_n = 0, recv_n = 0;
    std::vector<SubC> pack, unpack;
    /* chunked-exchange support (ordinary plans, one sub-block): the
     * send/recv blocks viewed as (rowelems x outer) with outer = the last
     * raw (Pi-mem-order + extras) axis — identical split on sender and
     * receiver by construction. */
    int64_t send_outer = 1, send_rowelems = 0;
    int64_t recv_outer = 1, recv_rowelems = 0;
    CopyDescH unpack_raw; /* un-normalized: nd = n+E, axis nd-1 = outer */
    bool has_unpack_raw = false;
};

struct StageTable; /* multi-field stage: launch list + device tables */

struct pa_plan {
    pa_pencil Pi, Po;
    int rank;
    int E;
    std::vector<int64_t> extra;
    int64_t esz;   /* bytes per element = ssz * ncomp */
    int64_t ssz;   /* bytes per scalar */
    int64_t ncomp; /* scalars per element, components fastest */
    /* reduced-precision wire (pa_plan_create_wire): the pair code, or 0.
     * Staging buffers and messages hold elements of msg_esz bytes — esz for
     * an ordinary plan, (wire scalar bytes) * ncomp for a wire plan. */
    int wire = 0;
    int64_t msg_esz;
    /* PA_PLAN_GROUP_CVT was given: on a wire plan the converting entries of
     * a stage share grouped launches (build_stage); no effect otherwise */
    bool group_cvt = false;
    /* PA_PLAN_GROUP_SOA was given: see pa_plan_group_soa() */
    bool group_soa = false;
    /* scaled transpose (pa_plan_set_scale): the PA_SCALAR_* code, or 0 for a
     * plan without a scale; an element is nscal such scalars.  The local
     * copy, the self unpack and the unpacks multiply by alpha, which is a
     * kernel argument and not part of the stage tables. */
    int scale = 0;
    int64_t nscal = 1;
    double alpha = 1.0;
    int R;    /* -1 = same decomposition */
    int P;    /* subgroup size */
    int myk;  /* my coordinate along R */
    std::vector<PeerBlockC> peers;
    /* the self block: fused src-window -> dst-window copies (`local`, no
     * staging block: off = n = 0), or in aliased (in-place) mode staged
     * through the recv tail (Transpositions.jl:250-264, :394-404) */
    bool aliased = false;
    std::vector<SubC> local, self_pack, self_unpack;
    int64_t send_total = 0, recv_total = 0; /* elements (remote blocks) */
    void *send_buf = nullptr, *recv_buf = nullptr;
    bool own_bufs = false;
    pa_comm *comm = nullptr;
    /* two-stream overlap: the exchange runs on comm_stream while the fused
     * local copy runs on the caller's stream (the reference overlaps the
     * local block with the exchange the same way: it copies it first and
     * unpacks it while recvs are in flight, Transpositions.jl:510-517). */
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_pack = nullptr, ev_comm = nullptr;
    /* >1: split the exchange into this many chunks and unpack each chunk
     * while later chunks are still in flight (the reference's Waitany
     * overlap, Transpositions.jl:510-517).  From PENCILHIP_EXCHANGE_CHUNKS;
     * default 1 (single grouped exchange). */
    int chunks = 1;
    std::vector<hipEvent_t> ev_chunks;
    /* per-stage timing (the TimerOutputs analogue, Transpositions.jl:
     * 173-177,327,337): opt-in HIP events with timing around pack / local /
     * exchange / unpack of the LAST execute.  tm[0..1] pack start/end and
     * tm[2] local end on the caller's stream; tm[3..4] exchange start/end on
     * the comm stream; tm[5..6] unpack start/end on the caller's stream. */
    bool timing = false;
    hipEvent_t tm[7] = {nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, nullptr};
    bool tm_valid[7] = {false, false, false, false, false, false, false};
    /* multi-field stages (pa_transpose_*_many): LRU of built stage tables,
     * keyed on (n, stage, every pointer the stage touches) */
    std::vector<StageTable *> tables;
    uint64_t table_clock = 0;
    int64_t table_builds = 0; /* tables ever built (pa_plan_stage_table_builds) */
    /* truncated transpose (pa_plan_create_keep): K_d = [0, keep_lo[d]) U
     * [N_d - keep_hi[d], N_d) per logical dim.  Every count and offset above
     * is then in KEPT elements and a block holds one sub-block per non-empty
     * sub-box; fills lists the destination windows outside the keep set
     * (PA_FILL_ZERO). */
    bool keep = false;
    int fill = PA_FILL_NONE;
    std::vector<int64_t> keep_lo, keep_hi;
    std::vector<FillDescH> fills;
};

static void free_stage_tables(pa_plan *p);

/* one descriptor of a plan: the ordinary copy, or on a wire plan the
 * converting copy with the op its stage calls for (op is ignored otherwise) */
static pa_status plan_launch(const pa_plan *p, int op, const CopyDescH &d,
                             const void *src, void *dst, hipStream_t stream)
{
    if (p->wire)
        return launch_desc_cvt(d, p->wire, op, p->ncomp, src, dst, stream);
    return launch_desc(d, p->ssz, p->ncomp, src, dst, stream);
}

static int64_t prod_extra(const pa_plan &pl)
{
    int64_t v = 1;
    for (auto e : pl.extra) v *= e;
    return v;
}

/* parent memory dims (memory-order local sizes + extra) and column-major
 * strides (axis 0 fastest — the Julia parent, arrays.jl:134-138). */
static void parent_strides(const pa_pencil &p, int rank,
                           const std::vector<int64_t> &extra, int64_t *mem,
                           int64_t *st, int *knd)
{
    Range ax[MAXND];
    axes_for_rank(p, rank, ax);
    int k = 0;
    for (int i = 0; i < p.n; i++, k++)
        mem[k] = ax[p.perm[i]].hi - ax[p.perm[i]].lo;
    for (auto e : extra) mem[k++] = e;
    int64_t acc = 1;
    for (int i = 0; i < k; i++) {
        st[i] = acc;
        acc *= mem[i];
    }
    *knd = k;
}

/* window of a global region in the parent of pencil p (axes in p's memory
 * order + extras): dims/strides/offset (to_local, Pencils.jl:579-587). */
static void window_desc(const pa_pencil &p, int rank,
                        const std::vector<int64_t> &extra, const Range *region,
                        int64_t *dims, int64_t *str, int64_t *off, int *knd)
{
    Range ax[MAXND];
    axes_for_rank(p, rank, ax);
    int64_t mem[2 * MAXND], pst[2 * MAXND];
    int k;
    parent_strides(p, rank, extra, mem, pst, &k);
    int64_t o = 0;
    for (int i = 0; i < p.n; i++) {
        const int d = p.perm[i];
        dims[i] = region[d].hi - region[d].lo;
        o += (region[d].lo - ax[d].lo) * pst[i];
    }
    for (size_t e = 0; e < extra.size(); e++) dims[p.n + e] = extra[e];
    for (int i = 0; i < k; i++) str[i] = pst[i];
    *off = o;
    *knd = k;
}

/* buffer->dest unpack descriptor: buffer axes = Pi memory order (+extras),
 * column-major with given strides; dest axis i' reads buffer axis
 * inv(perm_i)[perm_o[i']] (the relative permutation, Transpositions.jl:506).
 * raw_out, if given, receives the same copy un-normalized. */
static CopyDescH unpack_desc(const pa_plan &pl, const Range *grange,
                             const int64_t *bufdims, const int64_t *bufstr,
                             int64_t bufoff, CopyDescH *raw_out = nullptr)
{
    const pa_pencil &Po = pl.Po;
    const pa_pencil &Pi = pl.Pi;
    const int n = Pi.n;
    const int E = pl.E;

    Range axo[MAXND];
    axes_for_rank(Po, pl.rank, axo);
    int64_t mem_o[2 * MAXND], pst_o[2 * MAXND];
    int k;
    parent_strides(Po, pl.rank, pl.extra, mem_o, pst_o, &k);

    int32_t ipi[MAXND];
    for (int i = 0; i < n; i++) ipi[Pi.perm[i]] = i;

    int64_t dstr[2 * MAXND], doff = 0;
    for (int ip = 0; ip < n; ip++) {
        const int d = Po.perm[ip];
        dstr[ipi[d]] = pst_o[ip];
        doff += (grange[d].lo - axo[d].lo) * pst_o[ip];
    }
    for (int e = 0; e < E; e++) dstr[n + e] = pst_o[n + e];

    if (raw_out) {
        raw_out->nd = n + E;
        for (int i = 0; i < n + E; i++) {
            raw_out->dims[i] = bufdims[i];
            raw_out->sstr[i] = bufstr[i];
            raw_out->dstr[i] = dstr[i];
        }
        raw_out->soff = bufoff;
        raw_out->doff = doff;
        raw_out->total = 1;
        for (int i = 0; i < n + E; i++) raw_out->total *= bufdims[i];
    }
    return normalize_desc(n + E, bufdims, bufstr, bufoff, dstr, doff);
}


/* chunk of a raw (un-normalized) unpack descriptor: outer rows [lo, hi) of
 * its last axis */
static CopyDescH chunk_of_raw(const CopyDescH &raw, int64_t lo, int64_t hi)
{
    const int last = raw.nd - 1;
    int64_t dims[2 * MAXND], sstr[2 * MAXND], dstr[2 * MAXND];
    for (int i = 0; i < raw.nd; i++) {
        dims[i] = raw.dims[i];
        sstr[i] = raw.sstr[i];
        dstr[i] = raw.dstr[i];
    }
    dims[last] = hi - lo;
    return normalize_desc(raw.nd, dims, sstr, raw.soff + lo * sstr[last],
                          dstr, raw.doff + lo * dstr[last]);
}

static inline int64_t chunk_lo(int64_t outer, int c, int C)
{
    return outer * c / C;
}

/* ---- truncated transposes: sub-boxes of a block under a keep set ------ */

struct Box { Range r[MAXND]; };

/* the ranges of K_d, low before high; adjacent ranges merge */
static std::vector<Range> keep_ranges(int64_t a, int64_t b, int64_t N)
{
    if (a + b >= N) return {Range{0, N}};
    return {Range{0, a}, Range{N - b, N}};
}

/* every combination of one range per dim clipped to `clip`, dim 0 varying
 * fastest, empty boxes dropped */
static void box_product(int n, const std::vector<Range> *per_dim,
                        const Range *clip, std::vector<Box> *out)
{
    int idx[MAXND] = {0};
    while (true) {
        Box b;
        bool empty = false;
        for (int d = 0; d < n; d++) {
            range_intersect(per_dim[d][idx[d]], clip[d], &b.r[d]);
            if (b.r[d].hi <= b.r[d].lo) empty = true;
        }
        if (!empty) out->push_back(b);
        int d = 0;
        for (; d < n; d++) {
            if (++idx[d] < (int)per_dim[d].size()) break;
            idx[d] = 0;
        }
        if (d == n) return;
    }
}

/* The sub-boxes of a block.  Under a keep set: the non-empty intersections of
 * its region with K.  On an ordinary plan K is everything, so the region
 * itself, gated as ordinary plans always were: a block of a subgroup on its
 * element count, extras included, and the same-decomposition block (R < 0)
 * on its geometry alone. */
static void sub_boxes(const pa_plan &pl, const Range *region,
                      std::vector<Box> *out)
{
    const int n = pl.Pi.n;
    if (!pl.keep) {
        Box b;
        memcpy(b.r, region, sizeof(Range) * n);
        if (region_nelem(n, region) * (pl.R < 0 ? 1 : prod_extra(pl)) > 0)
            out->push_back(b);
        return;
    }
    std::vector<Range> per_dim[MAXND];
    for (int d = 0; d < n; d++)
        per_dim[d] = keep_ranges(pl.keep_lo[d], pl.keep_hi[d],
                                 pl.Pi.size_global[d]);
    box_product(n, per_dim, region, out);
}

static int64_t box_nelem(const pa_plan &pl, const Box &b)
{
    return region_nelem(pl.Pi.n, b.r) * prod_extra(pl);
}

/* pack of a box: src window -> column-major staging block at `off` */
static SubC pack_sub(const pa_plan &pl, const Box &b, int64_t off)
{
    int64_t dims[2 * MAXND], str[2 * MAXND], woff;
    int kk;
    window_desc(pl.Pi, pl.rank, pl.extra, b.r, dims, str, &woff, &kk);
    int64_t cstr[2 * MAXND], acc = 1;
    for (int i = 0; i < kk; i++) {
        cstr[i] = acc;
        acc *= dims[i];
    }
    return SubC{off, box_nelem(pl, b),
                normalize_desc(kk, dims, str, woff, cstr, off)};
}

/* unpack of a box: staging block at `off` (Pi memory order) -> dst window;
 * raw_out as in unpack_desc */
static SubC unpack_sub(const pa_plan &pl, const Box &b, int64_t off,
                       CopyDescH *raw_out = nullptr)
{
    const int n = pl.Pi.n, e = pl.E;
    int64_t bdims[2 * MAXND], bstr[2 * MAXND], acc = 1;
    for (int i = 0; i < n; i++)
        bdims[i] = b.r[pl.Pi.perm[i]].hi - b.r[pl.Pi.perm[i]].lo;
    for (int e2 = 0; e2 < e; e2++) bdims[n + e2] = pl.extra[e2];
    for (int i = 0; i < n + e; i++) {
        bstr[i] = acc;
        acc *= bdims[i];
    }
    return SubC{off, box_nelem(pl, b),
                unpack_desc(pl, b.r, bdims, bstr, off, raw_out)};
}

/* fused local copy of a box: src window -> dst window, no staging block */
static SubC local_sub(const pa_plan &pl, const Box &b)
{
    int64_t dims[2 * MAXND], str[2 * MAXND], off;
    int kk;
    window_desc(pl.Pi, pl.rank, pl.extra, b.r, dims, str, &off, &kk);
    return SubC{0, 0, unpack_desc(pl, b.r, dims, str, off)};
}

/* the self block: fused copies, or in aliased mode staged through the recv
 * buffer from element offset `off`; returns the end offset */
static int64_t self_block(pa_plan *pl, const Range *region, int64_t off)
{
    std::vector<Box> boxes;
    sub_boxes(*pl, region, &boxes);
    for (auto &b : boxes) {
        if (pl->aliased) {
            pl->self_pack.push_back(pack_sub(*pl, b, off));
            pl->self_unpack.push_back(unpack_sub(*pl, b, off));
            off += box_nelem(*pl, b);
        } else
            pl->local.push_back(local_sub(*pl, b));
    }
    return off;
}

/* The complement of the keep set inside this rank's destination range: for
 * d = 0..N-1, (kept in dims < d) x (dropped range of dim d) x (everything in
 * dims > d), as windows of the output parent. */
static void keep_fills(pa_plan *pl)
{
    const pa_pencil &Po = pl->Po;
    const int n = Po.n;
    if (prod_extra(*pl) == 0) return;
    Range axo[MAXND];
    axes_for_rank(Po, pl->rank, axo);
    int64_t mem_o[2 * MAXND], pst_o[2 * MAXND];
    int k;
    parent_strides(Po, pl->rank, pl->extra, mem_o, pst_o, &k);
    for (int d = 0; d < n; d++) {
        const int64_t a = pl->keep_lo[d], N = Po.size_global[d];
        const int64_t hi = N - pl->keep_hi[d];
        if (hi <= a) continue;
        std::vector<Range> per_dim[MAXND];
        for (int j = 0; j < n; j++) {
            if (j < d)
                per_dim[j] = keep_ranges(pl->keep_lo[j], pl->keep_hi[j],
                                         Po.size_global[j]);
            else if (j == d)
                per_dim[j] = {Range{a, hi}};
            else
                per_dim[j] = {Range{0, Po.size_global[j]}};
        }
        std::vector<Box> boxes;
        box_product(n, per_dim, axo, &boxes);
        for (auto &b : boxes) {
            int64_t dims[2 * MAXND], off = 0;
            for (int i = 0; i < n; i++) {
                const int ld = Po.perm[i];
                dims[i] = b.r[ld].hi - b.r[ld].lo;
                off += (b.r[ld].lo - axo[ld].lo) * pst_o[i];
            }
            for (int e = 0; e < pl->E; e++) dims[n + e] = pl->extra[e];
            pl->fills.push_back(normalize_fill(n + pl->E, dims, pst_o, off));
        }
    }
}

/* the last raw axis (Pi memory order + extras) of a block: the axis a chunked
 * exchange splits */
static int64_t outer_extent(const pa_plan &pl, const Range *region)
{
    if (pl.E) return pl.extra[pl.E - 1];
    const Range &r = region[pl.Pi.perm[pl.Pi.n - 1]];
    return r.hi - r.lo;
}

/* The one plan builder.  keep_lo/keep_hi null: an ordinary plan, every block
 * at most one sub-block; else the plan of a truncated transpose with `fill`.
 * Peers, their order and the staging layout are the same either way. */
static pa_status plan_build(const pa_pencil *pin, const pa_pencil *pout,
                            int64_t scalar_size, int64_t ncomp, int e,
                            const int64_t *extra_dims, int rank, int flags,
                            const int64_t *keep_lo, const int64_t *keep_hi,
                            int fill, pa_plan **out)
{
    /* assert_compatible (Transpositions.jl:182-199) */
    if (pin->topo.m != pout->topo.m || pin->topo.dims != pout->topo.dims)
        return fail("pencil topologies must be the same.");
    if (pin->n != pout->n || pin->size_global != pout->size_global)
        return fail("global data sizes must be the same between different "
                    "pencil configurations.");
    int ndiff = 0, R = -1;
    for (int j = 0; j < pin->topo.m; j++)
        if (pin->decomp[j] != pout->decomp[j]) {
            ndiff++;
            if (R < 0) R = j;
        }
    if (ndiff > 1)
        return fail("pencil decompositions must differ in at most one "
                    "dimension.");
    if (rank < 0 || rank >= pin->topo.nranks) return fail("rank out of range");
    if (pa_status cst = check_comp(scalar_size, ncomp)) return cst;
    if (pin->n + e > MAXND)
        return fail("too many dims: N+E must be <= %d", MAXND);

    const int n = pin->n;
    auto *pl = new pa_plan;
    pl->Pi = *pin;
    pl->Po = *pout;
    pl->rank = rank;
    pl->E = e;
    if (e) pl->extra.assign(extra_dims, extra_dims + e);
    pl->esz = scalar_size * ncomp;
    pl->ssz = scalar_size;
    pl->ncomp = ncomp;
    pl->msg_esz = pl->esz;
    pl->R = R;
    pl->aliased = (flags & PA_PLAN_ALIASED) != 0;
    pl->group_cvt = (flags & PA_PLAN_GROUP_CVT) != 0;
    pl->group_soa = (flags & PA_PLAN_GROUP_SOA) != 0;
    if (keep_lo) {
        /* the exchange of a keep plan is always a single group */
        pl->keep = true;
        pl->fill = fill;
        pl->keep_lo.assign(keep_lo, keep_lo + n);
        pl->keep_hi.assign(keep_hi, keep_hi + n);
        if (fill == PA_FILL_ZERO) keep_fills(pl);
    } else if (const char *ce = getenv("PENCILHIP_EXCHANGE_CHUNKS")) {
        int c = atoi(ce);
        if (c >= 1 && c <= 64) pl->chunks = c;
    }
    *out = pl;

    Range axl_i[MAXND], axl_o[MAXND];
    axes_for_rank(*pin, rank, axl_i);
    axes_for_rank(*pout, rank, axl_o);
    if (R < 0) {
        /* local path (transpose_impl!(::Nothing), Transpositions.jl:214-271;
         * aliased variant stages through recv_buf, :250-264) */
        pl->P = 1;
        pl->myk = 0;
        pl->recv_total = self_block(pl, axl_i, 0);
        return 0;
    }

    pl->P = (int)pin->topo.dims[R];
    int64_t coords[MAXND];
    cart_coords(pin->topo, rank, coords);
    pl->myk = (int)coords[R];

    Range self_region[MAXND];
    int64_t isend = 0, irecv = 0;
    for (int k = 0; k < pl->P; k++) {
        int64_t pc[MAXND];
        memcpy(pc, coords, sizeof(int64_t) * pin->topo.m);
        pc[R] = k;
        PeerBlockC blk;
        blk.k = k;
        blk.grank = cart_rank(pin->topo, pc);

        Range axp_o[MAXND], axp_i[MAXND], sr[MAXND], rr[MAXND];
        axes_for_coords(*pout, pc, axp_o);
        axes_for_coords(*pin, pc, axp_i);
        for (int d = 0; d < n; d++) {
            range_intersect(axl_i[d], axp_o[d], &sr[d]); /* :383 */
            range_intersect(axl_o[d], axp_i[d], &rr[d]); /* :388,:521 */
        }
        std::vector<Box> sb, rb;
        sub_boxes(*pl, sr, &sb);
        sub_boxes(*pl, rr, &rb);
        for (auto &b : sb) blk.send_n += box_nelem(*pl, b);
        for (auto &b : rb) blk.recv_n += box_nelem(*pl, b);
        if (k == pl->myk) {
            /* the self block (sr == rr) is never a message: fused, or staged
             * at the recv tail once the remote blocks are laid out */
            memcpy(self_region, sr, sizeof(Range) * n);
        } else {
            /* pack: column-major staging blocks in Pi memory order
             * (:346-431); unpack: the same blocks scattered by the relative
             * permutation (:527,:599-600) */
            blk.send_off = isend;
            blk.recv_off = irecv;
            for (auto &b : sb) {
                blk.pack.push_back(pack_sub(*pl, b, isend));
                isend += blk.pack.back().n;
            }
            for (auto &b : rb) {
                blk.unpack.push_back(unpack_sub(
                    *pl, b, irecv, pl->keep ? nullptr : &blk.unpack_raw));
                irecv += blk.unpack.back().n;
            }
            /* only an ordinary plan may chunk its exchange: its one
             * sub-block is the whole block, and non-empty */
            if (!pl->keep && !sb.empty()) {
                blk.send_outer = outer_extent(*pl, sr);
                blk.send_rowelems = blk.send_n / blk.send_outer;
            }
            if (!pl->keep && !rb.empty()) {
                blk.has_unpack_raw = true;
                blk.recv_outer = outer_extent(*pl, rr);
                blk.recv_rowelems = blk.recv_n / blk.recv_outer;
            }
        }
        pl->peers.push_back(blk);
    }
    pl->send_total = isend;
    /* fused self path: direct window->window permuted copy (replaces
     * :394-404 + :588-606; same values, half the HBM traffic).  Aliased
     * (in-place) mode stages the self block at the END of the recv buffer
     * like the reference, so every src read precedes any dst write. */
    if (pl->aliased) pl->peers[pl->myk].recv_off = irecv;
    pl->recv_total = self_block(pl, self_region, irecv);
    return 0;
}

/* ---- reading the block tables --------------------------------------- */

/* the sub-block list behind (which, k): 0 local, 1 pack of peer k, 2 unpack
 * of peer k, 3 staged self pack, 4 staged self unpack; null for any other
 * which or a peer the plan does not have */
static const std::vector<SubC> *block_list(const pa_plan *p, int which, int k)
{
    if (which == 0) return &p->local;
    if (which == 3) return &p->self_pack;
    if (which == 4) return &p->self_unpack;
    if (p->R < 0 || k < 0 || k >= (int)p->peers.size()) return nullptr;
    if (which == 1) return &p->peers[k].pack;
    if (which == 2) return &p->peers[k].unpack;
    return nullptr;
}

/* Multi-field staging layout: a staging block at element offset o with c
 * elements in the single-field plan holds field f of n at n*o + f*c; this is
 * how far that moves the block's staging-side offset. */
static inline int64_t many_shift(int n, int f, int64_t o, int64_t c)
{
    return (int64_t)(n - 1) * o + (int64_t)f * c;
}

static pa_status check_field(int n, int f)
{
    if (n < 1) return fail("n must be >= 1");
    if (f < 0 || f >= n) return fail("field %d out of range", f);
    return 0;
}

/* sub-block s of (which, k) for field f of n: its descriptor with the
 * staging side (dst of a pack, src of an unpack) moved by many_shift */
static pa_status field_desc(const pa_plan *p, int n, int f, int which, int k,
                            int s, CopyDescH *out)
{
    if (pa_status st = check_field(n, f)) return st;
    if (which < 0 || which > 4) return fail("bad which %d", which);
    const std::vector<SubC> *l = block_list(p, which, k);
    if (!l || s < 0 || s >= (int)l->size())
        return fail("no sub-box %d (which %d, peer %d)", s, which, k);
    const SubC &sb = (*l)[s];
    *out = sb.d;
    const int64_t sh = many_shift(n, f, sb.off, sb.n);
    if (which == 1 || which == 3)
        out->doff += sh;
    else
        out->soff += sh;
    return 0;
}

/* the one descriptor of (which, k) on an ordinary plan, or the error naming
 * what the plan lacks; `staged` words the missing self block for which 3/4 */
static pa_status single_desc(const pa_plan *p, int n, int f, int which, int k,
                             const char *const staged[2], CopyDescH *out)
{
    if (pa_status st = check_field(n, f)) return st;
    const std::vector<SubC> *l = block_list(p, which, k);
    if (l && !l->empty()) return field_desc(p, n, f, which, k, 0, out);
    if (which == 0) return fail("no local copy in plan");
    if (which == 3 || which == 4)
        return fail("no staged self %s in plan", staged[which - 3]);
    if (p->R < 0 || k < 0 || k >= (int)p->peers.size())
        return fail("no peer block %d", k);
    if (which == 1) return fail("no pack for peer %d", k);
    if (which == 2) return fail("no unpack for peer %d", k);
    return fail("bad which %d", which);
}

static pa_status keep_has_no_single(void)
{
    return fail("a keep plan has one descriptor per sub-box: use "
                "pa_plan_copydesc_sub");
}

static void copy_out(const CopyDescH &d, int64_t *nd, int64_t *dims,
                     int64_t *sstr, int64_t *soff, int64_t *dstr,
                     int64_t *doff)
{
    *nd = d.nd;
    for (int i = 0; i < d.nd; i++) {
        dims[i] = d.dims[i];
        sstr[i] = d.sstr[i];
        dstr[i] = d.dstr[i];
    }
    *soff = d.soff;
    *doff = d.doff;
}

/* ---- what the two executes share ------------------------------------ */

/* record timing event i on strm (pa_plan_enable_timing) */
#define TM_REC(i, strm)                                                      \
    do {                                                                     \
        if (p->timing) {                                                     \
            HIP_CHECK(hipEventRecord(p->tm[i], strm));                       \
            p->tm_valid[i] = true;                                           \
        }                                                                    \
    } while (0)

static pa_status timing_begin(pa_plan *p)
{
    if (!p->timing) return 0;
    for (auto &e : p->tm)
        if (!e) HIP_CHECK(hipEventCreate(&e));
    for (auto &v : p->tm_valid) v = false;
    return 0;
}

/* does this rank send or receive any message? */
static bool exchanging(const pa_plan *p)
{
    if (p->R >= 0 && p->P > 1)
        for (auto &blk : p->peers)
            if (blk.k != p->myk && (blk.send_n || blk.recv_n)) return true;
    return false;
}

static pa_status ensure_comm_stream(pa_plan *p)
{
    if (p->comm_stream) return 0;
    HIP_CHECK(hipStreamCreateWithFlags(&p->comm_stream,
                                       hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&p->ev_pack, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&p->ev_comm, hipEventDisableTiming));
    return 0;
}

extern "C" {

/* ---- topology ----------------------------------------------------- */

pa_status pa_topology_create(int m, const int64_t *pdims, pa_topology **out)
{
    if (m <= 0 || m > MAXND) return fail("invalid topology ndims %d", m);
    auto *t = new pa_topology;
    t->m = m;
    t->nranks = 1;
    for (int i = 0; i < m; i++) {
        if (pdims[i] <= 0) { delete t; return fail("invalid pdims"); }
        t->dims.push_back(pdims[i]);
        t->nranks *= pdims[i];
    }
    *out = t;
    return 0;
}

void pa_topology_destroy(pa_topology *t) { delete t; }
int pa_topology_nranks(const pa_topology *t) { return (int)t->nranks; }

pa_status pa_topology_coords(const pa_topology *t, int rank, int64_t *coords)
{
    if (rank < 0 || rank >= t->nranks) return fail("rank out of range");
    cart_coords(*t, rank, coords);
    return 0;
}

/* ---- pencil ------------------------------------------------------- */

pa_status pa_pencil_create(pa_topology *t, int n, const int64_t *size_global,
                           const int32_t *decomp_dims, const int32_t *perm,
                           pa_pencil **out)
{
    if (n <= 0 || n + 2 > MAXND) return fail("invalid ndims %d", n);
    if (t->m > n) return fail("M (%d) cannot exceed N (%d)", t->m, n);
    auto *p = new pa_pencil;
    p->topo = *t;
    p->n = n;
    p->size_global.assign(size_global, size_global + n);
    p->decomp.assign(decomp_dims, decomp_dims + t->m);
    /* _check_selected_dimensions (Pencils.jl:393-406) */
    for (int j = 0; j < t->m; j++) {
        if (p->decomp[j] < 0 || p->decomp[j] >= n) {
            delete p;
            return fail("decomp dim %d out of range", p->decomp[j]);
        }
        for (int j2 = 0; j2 < j; j2++)
            if (p->decomp[j2] == p->decomp[j]) {
                delete p;
                return fail("repeated decomp dim %d", p->decomp[j]);
            }
    }
    if (perm) {
        p->perm.assign(perm, perm + n);
        std::vector<int> seen(n, 0);
        for (int i = 0; i < n; i++) {
            if (p->perm[i] < 0 || p->perm[i] >= n || seen[p->perm[i]]++) {
                delete p;
                return fail("invalid permutation");
            }
        }
    } else {
        for (int i = 0; i < n; i++) p->perm.push_back(i);
    }
    *out = p;
    return 0;
}

void pa_pencil_destroy(pa_pencil *p) { delete p; }

pa_status pa_pencil_range_local(const pa_pencil *p, int rank, int memory_order,
                                int64_t *lo, int64_t *hi)
{
    if (rank < 0 || rank >= p->topo.nranks) return fail("rank out of range");
    Range ax[MAXND];
    axes_for_rank(*p, rank, ax);
    for (int i = 0; i < p->n; i++) {
        const int d = memory_order ? p->perm[i] : i;
        lo[i] = ax[d].lo;
        hi[i] = ax[d].hi;
    }
    return 0;
}

pa_status pa_pencil_size_local(const pa_pencil *p, int rank, int memory_order,
                               int64_t *out)
{
    int64_t lo[MAXND], hi[MAXND];
    pa_status st = pa_pencil_range_local(p, rank, memory_order, lo, hi);
    if (st) return st;
    for (int i = 0; i < p->n; i++) out[i] = hi[i] - lo[i];
    return 0;
}

int64_t pa_pencil_length_local(const pa_pencil *p, int rank)
{
    Range ax[MAXND];
    axes_for_rank(*p, rank, ax);
    return region_nelem(p->n, ax);
}

/* ---- comm --------------------------------------------------------- */

int pa_unique_id_size(void) { return (int)sizeof(ncclUniqueId); }

pa_status pa_get_unique_id(char *id)
{
    NCCL_CHECK(ncclGetUniqueId((ncclUniqueId *)id));
    return 0;
}

pa_status pa_comm_create(const char *id, int nranks, int rank, pa_comm **out)
{
    auto *c = new pa_comm;
    c->nranks = nranks;
    c->rank = rank;
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    /* Non-blocking init with a bounded wait: a blocking ncclCommInitRank
     * hangs forever if any subgroup rank is missing or disagrees — in an
     * unattended multi-process run that is an undiagnosable timeout.
     * Timeout via PENCILHIP_COMM_TIMEOUT_S (default 180 s). */
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    ncclResult_t r = ncclCommInitRankConfig(&c->comm, nranks, uid, rank, &cfg);
    if (r != ncclSuccess && r != ncclInProgress) {
        delete c;
        return fail("ncclCommInitRank: %s", ncclGetErrorString(r));
    }
    double timeout_s = 180.0;
    if (const char *te = getenv("PENCILHIP_COMM_TIMEOUT_S")) {
        double v = atof(te);
        if (v > 0) timeout_s = v;
    }
    const auto t0 = std::chrono::steady_clock::now();
    ncclResult_t st = ncclInProgress;
    while (true) {
        ncclResult_t qr = ncclCommGetAsyncError(c->comm, &st);
        if (qr != ncclSuccess) {
            (void)ncclCommAbort(c->comm);
            delete c;
            return fail("ncclCommGetAsyncError: %s", ncclGetErrorString(qr));
        }
        if (st == ncclSuccess) break;
        if (st != ncclInProgress) {
            (void)ncclCommAbort(c->comm);
            delete c;
            return fail("ncclCommInitRank (async): %s",
                        ncclGetErrorString(st));
        }
        const double waited = std::chrono::duration<double>(
            std::chrono::steady_clock::now() - t0).count();
        if (waited > timeout_s) {
            (void)ncclCommAbort(c->comm);
            delete c;
            return fail("ncclCommInitRank timed out after %.0f s (subgroup "
                        "nranks=%d rank=%d): a peer is missing or "
                        "disagrees on the unique id", timeout_s, nranks,
                        rank);
        }
        sched_yield();
    }
    *out = c;
    return 0;
}

void pa_comm_destroy(pa_comm *c)
{
    if (!c) return;
    ncclCommDestroy(c->comm);
    delete c;
}

/* ---- plan --------------------------------------------------------- */

pa_status pa_plan_create(const pa_pencil *pin, const pa_pencil *pout,
                         int64_t elem_size, int e, const int64_t *extra_dims,
                         int rank, int flags, pa_plan **out)
{
    return pa_plan_create_comp(pin, pout, elem_size, 1, e, extra_dims, rank,
                               flags, out);
}

pa_status pa_plan_create_comp(const pa_pencil *pin, const pa_pencil *pout,
                              int64_t scalar_size, int64_t ncomp, int e,
                              const int64_t *extra_dims, int rank, int flags,
                              pa_plan **out)
{
    return plan_build(pin, pout, scalar_size, ncomp, e, extra_dims, rank,
                      flags, nullptr, nullptr, PA_FILL_NONE, out);
}

pa_status pa_plan_create_wire(const pa_pencil *pin, const pa_pencil *pout,
                              int wire, int64_t ncomp, int e,
                              const int64_t *extra_dims, int rank, int flags,
                              pa_plan **out)
{
    if (!out) return fail("null plan output");
    if (pa_status st = check_wire(wire, PA_WIRE_NARROW, ncomp)) return st;
    int64_t stored, wsz;
    wire_sizes(wire, &stored, &wsz);
    /* the same tables as the plan of the stored type; only byte sizes differ */
    pa_plan *pl = nullptr;
    if (pa_status st = pa_plan_create_comp(pin, pout, stored, ncomp, e,
                                           extra_dims, rank, flags, &pl))
        return st;
    pl->wire = wire;
    pl->msg_esz = wsz * ncomp;
    pl->chunks = 1; /* the exchange of a wire plan is always a single group */
    *out = pl;
    return 0;
}

int pa_plan_wire(const pa_plan *p) { return p ? p->wire : 0; }

int pa_plan_group_cvt(const pa_plan *p)
{
    return p && p->wire && p->group_cvt ? 1 : 0;
}

int pa_plan_group_soa(const pa_plan *p)
{
    return p && p->group_soa && !p->aliased && !p->wire && p->ncomp == 1 &&
                   (p->ssz == 4 || p->ssz == 8 || p->ssz == 16)
               ? 1
               : 0;
}

pa_status pa_plan_set_scale(pa_plan *p, int scalar, double alpha)
{
    if (!p) return fail("null plan");
    if (p->wire)
        return fail("a plan with a wire pair takes no scale: that would be "
                    "two roundings per element");
    if (pa_status st = check_scale(scalar, 1, alpha)) return st;
    const int64_t sz = scalar_bytes(scalar);
    if (p->esz % sz)
        return fail("element size %lld is not a multiple of the %lld-byte "
                    "scalar", (long long)p->esz, (long long)sz);
    /* alpha == 1 is "no scale": the plan runs what it runs without one */
    const int scale = alpha == 1.0 ? 0 : scalar;
    /* the tables hold the kernel selection, not alpha: they survive a change
     * of alpha and go when the selection changes */
    if (scale != p->scale) free_stage_tables(p);
    p->scale = scale;
    p->nscal = scale ? p->esz / sz : 1;
    p->alpha = scale ? alpha : 1.0;
    return 0;
}

int pa_plan_scale(const pa_plan *p, int *scalar, double *alpha)
{
    if (!p || !p->scale) return 0;
    if (scalar) *scalar = p->scale;
    if (alpha) *alpha = p->alpha;
    return 1;
}

pa_status pa_plan_create_keep(const pa_pencil *pin, const pa_pencil *pout,
                              int64_t scalar_size, int64_t ncomp, int e,
                              const int64_t *extra_dims, int rank, int flags,
                              const int64_t *keep_lo, const int64_t *keep_hi,
                              int fill, pa_plan **out)
{
    if (!out || !pin || !pout) return fail("null argument");
    if (!keep_lo || !keep_hi) return fail("null keep_lo / keep_hi");
    if (fill != PA_FILL_NONE && fill != PA_FILL_ZERO)
        return fail("fill must be PA_FILL_NONE (0) or PA_FILL_ZERO (1), got %d",
                    fill);
    for (int d = 0; d < pin->n; d++)
        if (keep_lo[d] < 0 || keep_hi[d] < 0 ||
            keep_lo[d] + keep_hi[d] > pin->size_global[d])
            return fail("keep set of dim %d: (%lld, %lld) must satisfy a, b "
                        ">= 0 and a + b <= %lld", d, (long long)keep_lo[d],
                        (long long)keep_hi[d],
                        (long long)pin->size_global[d]);
    return plan_build(pin, pout, scalar_size, ncomp, e, extra_dims, rank,
                      flags, keep_lo, keep_hi, fill, out);
}

int pa_plan_keep(const pa_plan *p, int64_t *lo, int64_t *hi, int *fill)
{
    if (!p || !p->keep) return 0;
    for (size_t d = 0; d < p->keep_lo.size(); d++) {
        if (lo) lo[d] = p->keep_lo[d];
        if (hi) hi[d] = p->keep_hi[d];
    }
    if (fill) *fill = p->fill;
    return 1;
}

void pa_plan_destroy(pa_plan *p)
{
    if (!p) return;
    if (p->own_bufs) {
        if (p->send_buf) (void)hipFree(p->send_buf);
        if (p->recv_buf) (void)hipFree(p->recv_buf);
    }
    if (p->ev_pack) (void)hipEventDestroy(p->ev_pack);
    if (p->ev_comm) (void)hipEventDestroy(p->ev_comm);
    for (auto e : p->ev_chunks) (void)hipEventDestroy(e);
    for (auto e : p->tm)
        if (e) (void)hipEventDestroy(e);
    if (p->comm_stream) (void)hipStreamDestroy(p->comm_stream);
    free_stage_tables(p);
    delete p;
}

pa_status pa_plan_set_comm(pa_plan *p, pa_comm *c)
{
    if (p->R >= 0 && p->P > 1) {
        if (c->nranks != p->P)
            return fail("comm size %d != subgroup size %d", c->nranks, p->P);
        if (c->rank != p->myk)
            return fail("comm rank %d != my subgroup coordinate %d", c->rank,
                        p->myk);
    }
    p->comm = c;
    return 0;
}

pa_status pa_plan_buffer_sizes(const pa_plan *p, int64_t *send_bytes,
                               int64_t *recv_bytes)
{
    *send_bytes = p->send_total * p->msg_esz;
    *recv_bytes = p->recv_total * p->msg_esz;
    return 0;
}

pa_status pa_plan_set_buffers(pa_plan *p, void *send_buf, void *recv_buf)
{
    free_stage_tables(p); /* tables bake the staging pointers in */
    if (p->own_bufs) {
        if (p->send_buf) (void)hipFree(p->send_buf);
        if (p->recv_buf) (void)hipFree(p->recv_buf);
        p->own_bufs = false;
    }
    p->send_buf = send_buf;
    p->recv_buf = recv_buf;
    return 0;
}

pa_status pa_transpose_execute(pa_plan *p, const void *src_parent,
                               void *dst_parent, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;

    const bool need_bufs = p->send_total > 0 || p->recv_total > 0;
    if (need_bufs && !p->send_buf && !p->own_bufs) {
        if (p->send_total)
            HIP_CHECK(hipMalloc(&p->send_buf, p->send_total * p->msg_esz));
        if (p->recv_total)
            HIP_CHECK(hipMalloc(&p->recv_buf, p->recv_total * p->msg_esz));
        p->own_bufs = true;
    }

    /* a keep plan runs the n = 1 stage path: pack -> exchange -> local +
     * fill -> unpack (the fallback above is sized in kept elements); so does
     * a wire plan with grouped converting kernels (sized in wire bytes) and
     * a scaled plan, whose scaling kernels are grouped from the start */
    if (p->keep || pa_plan_group_cvt(p) || p->scale) {
        const void *srcs[1] = {src_parent};
        void *dsts[1] = {dst_parent};
        return pa_transpose_execute_many(p, 1, srcs, dsts, stream_);
    }

    if (pa_status st = timing_begin(p)) return st;

    /* 1. pack every remote block (Transpositions.jl:346-431); in aliased
     * mode also stage the self block into the recv tail before any dst
     * write (:394-404) */
    TM_REC(0, stream);
    for (auto &blk : p->peers)
        for (auto &sb : blk.pack)
            if (pa_status st = plan_launch(p, PA_WIRE_NARROW, sb.d,
                                           src_parent, p->send_buf, stream))
                return st;
    for (auto &sb : p->self_pack)
        if (pa_status st = plan_launch(p, PA_WIRE_NARROW, sb.d, src_parent,
                                       p->recv_buf, stream))
            return st;
    TM_REC(1, stream);

    /* 2. exchange: grouped ncclSend/ncclRecv over xGMI on a dedicated comm
     * stream ordered after the pack kernels (replaces :419-428/:463-479;
     * the pre-send device sync of :472-473 is unnecessary — everything is
     * stream/event-ordered).  The fused local copy (step 3) runs on the
     * caller's stream CONCURRENTLY with the exchange — the engine's
     * equivalent of the reference's unpack-local-while-recvs-fly overlap
     * (Transpositions.jl:510-517). */
    const bool xchg = exchanging(p);
    const int C = (xchg && p->chunks > 1) ? p->chunks : 1;
    if (xchg) {
        if (!p->comm)
            return fail("subgroup exchange requires pa_plan_set_comm");
        if (pa_status st = ensure_comm_stream(p)) return st;
        while ((int)p->ev_chunks.size() < C) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            p->ev_chunks.push_back(e);
        }
        HIP_CHECK(hipEventRecord(p->ev_pack, stream));
        HIP_CHECK(hipStreamWaitEvent(p->comm_stream, p->ev_pack, 0));
        TM_REC(3, p->comm_stream);
        /* C == 1: one grouped exchange.  C > 1: the exchange is split into C
         * groups of matching per-peer sub-blocks (outer rows of the block,
         * identical split on sender and receiver), and each chunk's unpack
         * overlaps the later chunks' transfers — the reference's Waitany
         * overlap (Transpositions.jl:510-517) in stream/event form. */
        for (int c = 0; c < C; c++) {
            NCCL_CHECK(ncclGroupStart());
            for (auto &blk : p->peers) {
                if (blk.k == p->myk) continue;
                if (blk.recv_n) {
                    const int64_t lo = chunk_lo(blk.recv_outer, c, C);
                    const int64_t hi = chunk_lo(blk.recv_outer, c + 1, C);
                    if (hi > lo)
                        NCCL_CHECK(ncclRecv(
                            (char *)p->recv_buf +
                                (blk.recv_off + lo * blk.recv_rowelems) *
                                    p->msg_esz,
                            (size_t)((hi - lo) * blk.recv_rowelems *
                                     p->msg_esz),
                            ncclUint8, blk.k, p->comm->comm, p->comm_stream));
                }
                if (blk.send_n) {
                    const int64_t lo = chunk_lo(blk.send_outer, c, C);
                    const int64_t hi = chunk_lo(blk.send_outer, c + 1, C);
                    if (hi > lo)
                        NCCL_CHECK(ncclSend(
                            (const char *)p->send_buf +
                                (blk.send_off + lo * blk.send_rowelems) *
                                    p->msg_esz,
                            (size_t)((hi - lo) * blk.send_rowelems *
                                     p->msg_esz),
                            ncclUint8, blk.k, p->comm->comm, p->comm_stream));
                }
            }
            NCCL_CHECK(ncclGroupEnd());
            HIP_CHECK(hipEventRecord(p->ev_chunks[c], p->comm_stream));
        }
        TM_REC(4, p->comm_stream);
        HIP_CHECK(hipEventRecord(p->ev_comm, p->comm_stream));
    }

    /* 3. fused local/self copy — on the caller's stream, overlapping the
     * exchange (aliased mode: unpack the staged self block instead) */
    for (auto &sb : p->local)
        if (pa_status st = plan_launch(p, PA_WIRE_ROUND, sb.d, src_parent,
                                       dst_parent, stream))
            return st;
    for (auto &sb : p->self_unpack)
        if (pa_status st = plan_launch(p, PA_WIRE_WIDEN, sb.d, p->recv_buf,
                                       dst_parent, stream))
            return st;
    TM_REC(2, stream);

    /* 4. unpack received blocks (:489-536).  C == 1: all after the single
     * exchange completes.  C > 1: chunk c unpacks as soon as its group
     * lands, overlapping chunks c+1.. in flight. */
    if (C <= 1) {
        if (xchg) HIP_CHECK(hipStreamWaitEvent(stream, p->ev_comm, 0));
        TM_REC(5, stream);
        for (auto &blk : p->peers)
            for (auto &sb : blk.unpack)
                if (pa_status st = plan_launch(p, PA_WIRE_WIDEN, sb.d,
                                               p->recv_buf, dst_parent,
                                               stream))
                    return st;
        TM_REC(6, stream);
    } else {
        for (int c = 0; c < C; c++) {
            HIP_CHECK(hipStreamWaitEvent(stream, p->ev_chunks[c], 0));
            if (c == 0) TM_REC(5, stream);
            for (auto &blk : p->peers) {
                if (!blk.has_unpack_raw) continue;
                const int64_t lo = chunk_lo(blk.recv_outer, c, C);
                const int64_t hi = chunk_lo(blk.recv_outer, c + 1, C);
                if (hi <= lo) continue;
                CopyDescH d = chunk_of_raw(blk.unpack_raw, lo, hi);
                pa_status st =
                    plan_launch(p, PA_WIRE_WIDEN, d, p->recv_buf, dst_parent,
                                stream);
                if (st) return st;
            }
        }
        TM_REC(6, stream);
    }
    return 0;
}

/* ---- per-stage timing (TimerOutputs analogue) ---------------------- */

pa_status pa_plan_enable_timing(pa_plan *p, int enable)
{
    p->timing = enable != 0;
    return 0;
}

pa_status pa_plan_stage_times(pa_plan *p, double out[4])
{
    /* Valid after the last execute has completed (pa_transpose_wait).
     * out = {pack_ms, local_ms, exchange_ms, unpack_ms}; -1 for stages the
     * plan does not have. */
    if (!p->timing) return fail("timing not enabled (pa_plan_enable_timing)");
    float ms;
    auto span = [&](int a, int b) -> double {
        if (!p->tm_valid[a] || !p->tm_valid[b]) return -1.0;
        if (hipEventElapsedTime(&ms, p->tm[a], p->tm[b]) != hipSuccess)
            return -1.0;
        return (double)ms;
    };
    out[0] = span(0, 1); /* pack (+ staged self pack)      */
    out[1] = span(1, 2); /* fused local / self unpack      */
    out[2] = span(3, 4); /* exchange (comm stream)         */
    out[3] = span(5, 6); /* unpack of received blocks      */
    return 0;
}

pa_status pa_transpose_wait(pa_plan *p, void *stream_)
{
    (void)p;
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_));
    return 0;
}

/* ---- introspection ------------------------------------------------ */

int pa_plan_nproc_sub(const pa_plan *p) { return p->P; }
int pa_plan_r_dim(const pa_plan *p) { return p->R; }
int pa_plan_my_k(const pa_plan *p) { return p->myk; }

pa_status pa_plan_block_info(const pa_plan *p, int k, int64_t out[8])
{
    if (p->R < 0 || k < 0 || k >= (int)p->peers.size())
        return fail("no peer block %d", k);
    const PeerBlockC &b = p->peers[k];
    out[0] = b.k;
    out[1] = b.grank;
    out[2] = b.send_off;
    out[3] = b.recv_off;
    out[4] = b.send_n;
    out[5] = b.recv_n;
    out[6] = !b.pack.empty();
    out[7] = !b.unpack.empty();
    return 0;
}

pa_status pa_plan_copydesc(const pa_plan *p, int which, int k, int64_t *nd,
                           int64_t *dims, int64_t *sstr, int64_t *soff,
                           int64_t *dstr, int64_t *doff)
{
    static const char *const staged[2] = {"pack", "unpack"};
    if (p->keep) return keep_has_no_single();
    CopyDescH d;
    if (which == 5) { /* raw (un-normalized) unpack: nd = n+E <= MAXND */
        if (p->R < 0 || k < 0 || k >= (int)p->peers.size())
            return fail("no peer block %d", k);
        if (!p->peers[k].has_unpack_raw) return fail("no raw unpack");
        d = p->peers[k].unpack_raw;
    } else if (pa_status st = single_desc(p, 1, 0, which, k, staged, &d))
        return st;
    copy_out(d, nd, dims, sstr, soff, dstr, doff);
    return 0;
}

/* ---- reductions ---------------------------------------------------- */

pa_status pa_allreduce(pa_comm *c, const void *sendbuf, void *recvbuf,
                       int64_t count, int dtype, int op, void *stream)
{
    static const ncclDataType_t dts[] = {ncclFloat64, ncclFloat32, ncclInt64,
                                         ncclInt32, ncclUint8};
    static const ncclRedOp_t ops[] = {ncclSum, ncclProd, ncclMin, ncclMax};
    if (dtype < 0 || dtype > 4) return fail("bad dtype %d", dtype);
    if (op < 0 || op > 3) return fail("bad op %d", op);
    NCCL_CHECK(ncclAllReduce(sendbuf, recvbuf, (size_t)count, dts[dtype],
                             ops[op], c->comm, (hipStream_t)stream));
    return 0;
}

/* ---- standalone device copy --------------------------------------- */

pa_status pa_device_copy(int nd, const int64_t *dims, const int64_t *sstr,
                         int64_t soff, const int64_t *dstr, int64_t doff,
                         int64_t elem_size, const void *src, void *dst,
                         void *stream)
{
    return pa_device_copy_comp(nd, dims, sstr, soff, dstr, doff, elem_size, 1,
                               src, dst, stream);
}

pa_status pa_device_copy_comp(int nd, const int64_t *dims,
                              const int64_t *sstr, int64_t soff,
                              const int64_t *dstr, int64_t doff,
                              int64_t scalar_size, int64_t ncomp,
                              const void *src, void *dst, void *stream)
{
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    CopyDescH d = normalize_desc(nd, dims, sstr, soff, dstr, doff);
    return launch_desc(d, scalar_size, ncomp, src, dst, (hipStream_t)stream);
}

pa_status pa_copy_kernel_kind(int nd, const int64_t *dims, const int64_t *sstr,
                              int64_t soff, const int64_t *dstr, int64_t doff,
                              int64_t elem_size, const void *src,
                              const void *dst, int64_t out[4])
{
    int64_t o5[5];
    pa_status st = pa_copy_kernel_kind_comp(nd, dims, sstr, soff, dstr, doff,
                                            elem_size, 1, src, dst, o5);
    if (st) return st;
    for (int i = 0; i < 4; i++) out[i] = o5[i];
    return 0;
}

pa_status pa_copy_kernel_kind_comp(int nd, const int64_t *dims,
                                   const int64_t *sstr, int64_t soff,
                                   const int64_t *dstr, int64_t doff,
                                   int64_t scalar_size, int64_t ncomp,
                                   const void *src, const void *dst,
                                   int64_t out[5])
{
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    if (scalar_size <= 0) return fail("bad elem_size");
    CopyDescH d = normalize_desc(nd, dims, sstr, soff, dstr, doff);
    KernelSel k;
    pa_status st = select_kernel_comp(d, scalar_size, ncomp, src, dst, &k);
    if (st) return st;
    out[0] = k.kind;
    out[1] = k.word;
    out[2] = k.byteified;
    out[3] = k.sweep;
    out[4] = k.m;
    return 0;
}

pa_status pa_copy_kernel_stream(int nd, const int64_t *dims,
                                const int64_t *sstr, int64_t soff,
                                const int64_t *dstr, int64_t doff,
                                int64_t elem_size, const void *src,
                                const void *dst, int64_t *out)
{
    if (!out) return fail("null output");
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    if (elem_size <= 0) return fail("bad elem_size");
    CopyDescH d = normalize_desc(nd, dims, sstr, soff, dstr, doff);
    KernelSel k;
    pa_status st = select_kernel_comp(d, elem_size, 1, src, dst, &k);
    if (st) return st;
    *out = k.stream;
    return 0;
}

int64_t pa_set_stream_min_bytes(int64_t min_bytes)
{
    return g_stream_min_bytes.exchange(min_bytes);
}

pa_status pa_device_copy_wire(int nd, const int64_t *dims,
                              const int64_t *sstr, int64_t soff,
                              const int64_t *dstr, int64_t doff, int wire,
                              int op, int64_t ncomp, const void *src,
                              void *dst, void *stream)
{
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    if (pa_status st = check_wire(wire, op, ncomp)) return st;
    CopyDescH d = normalize_desc(nd, dims, sstr, soff, dstr, doff);
    return launch_desc_cvt(d, wire, op, ncomp, src, dst,
                           (hipStream_t)stream);
}

pa_status pa_copy_kernel_kind_wire(int nd, const int64_t *dims,
                                   const int64_t *sstr, int64_t soff,
                                   const int64_t *dstr, int64_t doff,
                                   int wire, int op, int64_t ncomp,
                                   const void *src, const void *dst,
                                   int64_t out[5])
{
    if (!out) return fail("null output");
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    if (pa_status st = check_wire(wire, op, ncomp)) return st;
    CopyDescH d = normalize_desc(nd, dims, sstr, soff, dstr, doff);
    CvtSel k;
    if (pa_status st = select_kernel_cvt(d, wire, op, ncomp, src, dst, &k))
        return st;
    out[0] = k.kind;
    out[1] = k.V;
    out[2] = k.ti;
    out[3] = k.tj;
    out[4] = 1; /* the converting tile sweeps one tile per workgroup */
    return 0;
}

pa_status pa_device_copy_scale(int nd, const int64_t *dims,
                               const int64_t *sstr, int64_t soff,
                               const int64_t *dstr, int64_t doff, int scalar,
                               int64_t nscal, double alpha, const void *src,
                               void *dst, void *stream)
{
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    if (pa_status st = check_scale(scalar, nscal, alpha)) return st;
    CopyDescH d = normalize_desc(nd, dims, sstr, soff, dstr, doff);
    CvtSel k;
    if (pa_status st = select_kernel_scale(d, scalar, nscal, src, dst, &k))
        return st;
    return launch_scale_sel(k, src, dst, alpha, (hipStream_t)stream);
}

pa_status pa_copy_kernel_kind_scale(int nd, const int64_t *dims,
                                    const int64_t *sstr, int64_t soff,
                                    const int64_t *dstr, int64_t doff,
                                    int scalar, int64_t nscal,
                                    const void *src, const void *dst,
                                    int64_t out[5])
{
    if (!out) return fail("null output");
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    CopyDescH d = normalize_desc(nd, dims, sstr, soff, dstr, doff);
    CvtSel k;
    if (pa_status st = select_kernel_scale(d, scalar, nscal, src, dst, &k))
        return st;
    out[0] = k.kind;
    out[1] = k.V;
    out[2] = k.ti;
    out[3] = k.tj;
    out[4] = 1; /* the scaling tile sweeps one tile per workgroup */
    return 0;
}

} /* extern "C" */

/* ================= multi-field transposes ========================== */
/* n fields of one pencil pair in one call: one grouped launch per stage
 * and kernel signature, one message per peer carrying all n fields, and
 * the stages exposed separately so a host can run its own exchange.
 *
 * Staging layout: a staging block at element offset o with c elements in
 * the single-field plan holds field f at n*o + f*c.  Blocks are
 * consecutive, so this tiles the n-fold buffer exactly and peer k's message
 * is the contiguous range [n*o_k, n*(o_k + c_k)). */

enum {
    STAGE_PACK = PA_STAGE_PACK,
    STAGE_LOCAL = PA_STAGE_LOCAL,
    STAGE_UNPACK = PA_STAGE_UNPACK
};

/* the kernel family of a stage entry: which selection of the item runs */
enum Family { FAM_COPY, FAM_CVT, FAM_SCALE, FAM_SOA, FAM_FILL };

struct StageItem {
    Family fam = FAM_COPY;
    KernelSel k; /* FAM_COPY */
    CvtSel c;    /* FAM_CVT (wire plan), FAM_SCALE (a scaled plan's
                  * destination side) */
    SoaSel s;    /* FAM_SOA: on the vector-valued array aos and the field
                  * pointers (or staging slots) */
    FillSel fs;  /* FAM_FILL (keep plan) */
    void *aos = nullptr;
    std::vector<void *> fields;
    const void *src = nullptr;
    void *dst = nullptr;
    Grid g;
};

/* What the entries of one grouped launch have in common, compared whole; a
 * family sets the fields it does not use to 0. */
struct StageSig {
    int kind = 0;
    int word = 0; /* copy kinds: bytes per word */
    int op = 0;   /* converting kinds: wire op */
    int vec = 0;  /* linear converting, scaling and split / join kinds: V */
    bool operator==(const StageSig &o) const
    {
        return kind == o.kind && word == o.word && op == o.op && vec == o.vec;
    }
};

struct StageLaunch {
    StageSig sig;
    bool grouped = false;
    std::vector<int> items;
    int64_t nblocks = 0;
    void *d_mem = nullptr; /* grouped: first[nent] then the entries */
};

struct StageTable {
    std::vector<uintptr_t> key;
    std::vector<StageItem> items;
    std::vector<StageLaunch> launches;
    uint64_t stamp = 0;
};

#define PA_STAGE_TABLES_MAX 12

/* Append an entry: a groupable one joins the open grouped launch of its
 * signature, else it opens a new row, so rows stand in first-appearance
 * order.  An entry without workgroups is dropped. */
static void stage_push(StageTable *t, const StageItem &it,
                       const StageSig &sig, bool groupable)
{
    if (it.g.nblocks == 0) return;
    const int idx = (int)t->items.size();
    t->items.push_back(it);
    if (groupable)
        for (auto &l : t->launches)
            if (l.grouped && l.sig == sig) {
                l.items.push_back(idx);
                l.nblocks += it.g.nblocks;
                return;
            }
    StageLaunch l;
    l.sig = sig;
    l.grouped = groupable;
    l.items.push_back(idx);
    l.nblocks = it.g.nblocks;
    t->launches.push_back(l);
}

/* one copy entry: the grouped kernels cover the linear kinds and the
 * one-tile-per-workgroup tiles, per word; everything else launches alone */
static pa_status stage_add_copy(StageTable *t, const CopyDescH &d,
                                int64_t ssz, int64_t ncomp, const void *src,
                                void *dst)
{
    StageItem it;
    it.src = src;
    it.dst = dst;
    if (pa_status st = select_kernel_comp(d, ssz, ncomp, src, dst, &it.k))
        return st;
    const KernelSel &k = it.k;
    it.g = sel_grid(k);
    StageSig sig;
    sig.kind = k.kind;
    sig.word = k.word;
    bool grp = false;
    if (k.kind == PA_KERNEL_COPY_1D || k.kind == PA_KERNEL_LINEAR) {
        sig.kind = PA_KERNEL_LINEAR;
        grp = true;
    } else if (k.kind == PA_KERNEL_TILE || k.kind == PA_KERNEL_TILE_VS)
        grp = k.sweep == 1;
    stage_push(t, it, sig, grp);
    return 0;
}

/* one converting (fam FAM_CVT) or scaling (FAM_SCALE) entry, its selection
 * already in it->c: linear entries of one (op, V) and tile entries of one op
 * may share a grouped launch */
static void stage_add_cvt(StageTable *t, StageItem *it, bool grouped)
{
    const CvtSel &c = it->c;
    it->g.nblocks = cvt_grid(c, &it->g.nti, &it->g.njc);
    const bool lin = c.kind == PA_KERNEL_CVT_LINEAR ||
                     c.kind == PA_KERNEL_SCALE_LINEAR;
    const bool tile = c.kind == PA_KERNEL_CVT_TILE ||
                      c.kind == PA_KERNEL_SCALE_TILE;
    StageSig sig;
    sig.kind = c.kind;
    sig.op = c.op;
    sig.vec = lin ? c.V : 0;
    stage_push(t, *it, sig, grouped && (lin || tile));
}

/* one zero-fill entry of a window of esz-byte elements; all of a stage share
 * ONE grouped launch */
static pa_status stage_add_fill(StageTable *t, const FillDescH &d,
                                int64_t esz, void *dst)
{
    StageItem it;
    it.fam = FAM_FILL;
    it.dst = dst;
    if (pa_status st = select_fill(d, esz, dst, &it.fs)) return st;
    it.g.nblocks = it.fs.nblocks;
    StageSig sig;
    sig.kind = PA_KERNEL_FILL;
    stage_push(t, it, sig, true);
    return 0;
}

/* The launch list of one n-field stage: one copy (stage_add_copy()),
 * converting or scaling (stage_add_cvt()) entry per sub-block and field, then
 * a keep plan's fill entries; groupable entries of one StageSig share a
 * grouped launch (stage_push()).  Host-only; pointers are used for alignment
 * only. */
static pa_status build_stage(const pa_plan *p, int n, int stage,
                             const void *const *srcs, void *const *dsts,
                             const void *send_buf, void *recv_buf,
                             StageTable *t)
{
    auto add_desc = [&](const CopyDescH &d, int which, const void *src,
                        void *dst) -> pa_status {
        /* a scaled plan multiplies on the destination side only: the local
         * copy, the self unpack and the unpacks; its packs stay ordinary */
        const bool scaled = p->scale && (which == 0 || which == 2 || which == 4);
        if (!p->wire && !scaled)
            return stage_add_copy(t, d, p->ssz, p->ncomp, src, dst);
        StageItem it;
        it.src = src;
        it.dst = dst;
        if (scaled) {
            it.fam = FAM_SCALE;
            if (pa_status st = select_kernel_scale(d, p->scale, p->nscal, src,
                                                   dst, &it.c))
                return st;
        } else {
            const int op = which == 0 ? PA_WIRE_ROUND
                           : (which == 1 || which == 3) ? PA_WIRE_NARROW
                                                        : PA_WIRE_WIDEN;
            it.fam = FAM_CVT;
            if (pa_status st = select_kernel_cvt(d, p->wire, op, p->ncomp,
                                                 src, dst, &it.c))
                return st;
        }
        /* the converting kernels are grouped where the plan asks for it
         * (PA_PLAN_GROUP_CVT), the scaling kernels always */
        stage_add_cvt(t, &it, scaled || p->group_cvt);
        return 0;
    };
    /* every sub-block of `which` (of peer k) for field f */
    auto add = [&](int f, int which, int k, const void *src,
                   void *dst) -> pa_status {
        const std::vector<SubC> *l = block_list(p, which, k);
        for (int s = 0; l && s < (int)l->size(); s++) {
            CopyDescH d;
            if (pa_status st = field_desc(p, n, f, which, k, s, &d)) return st;
            if (pa_status st = add_desc(d, which, src, dst)) return st;
        }
        return 0;
    };
    auto add_fill = [&](const FillDescH &d, void *dst) -> pa_status {
        return stage_add_fill(t, d, p->esz, dst);
    };

    for (int f = 0; f < n; f++) {
        const void *src = srcs ? srcs[f] : nullptr;
        void *dst = dsts ? dsts[f] : nullptr;
        if (stage == STAGE_PACK) {
            for (auto &b : p->peers)
                if (pa_status st = add(f, 1, b.k, src, (void *)send_buf))
                    return st;
            if (pa_status st = add(f, 3, 0, src, recv_buf)) return st;
        } else if (stage == STAGE_LOCAL) {
            if (pa_status st = add(f, 0, 0, src, dst)) return st;
            if (pa_status st = add(f, 4, 0, recv_buf, dst)) return st;
        } else {
            for (auto &b : p->peers)
                if (pa_status st = add(f, 2, b.k, recv_buf, dst)) return st;
        }
    }
    /* the fill entries of every field (keep plans), after the copies of the
     * stage */
    if (stage == STAGE_LOCAL)
        for (int f = 0; f < n; f++)
            for (auto &fd : p->fills)
                if (pa_status st = add_fill(fd, dsts ? dsts[f] : nullptr))
                    return st;
    return 0;
}

static void free_table(StageTable *t)
{
    /* hipFree waits for the device, so no launch still reads the table */
    for (auto &l : t->launches)
        if (l.d_mem) (void)hipFree(l.d_mem);
    delete t;
}

static void free_stage_tables(pa_plan *p)
{
    for (auto *t : p->tables) free_table(t);
    p->tables.clear();
}

/* the device table of one grouped launch, first[nent] then E[nent]: a fresh
 * allocation and one blocking copy, never modified afterwards.  make(item)
 * is the entry of an item. */
template <typename E, typename Make>
static pa_status upload_launch(const StageTable &t, StageLaunch *l, Make make)
{
    const size_t ne = l->items.size();
    std::vector<char> host(ne * (sizeof(int64_t) + sizeof(E)));
    int64_t *first = (int64_t *)host.data();
    char *ent = host.data() + ne * sizeof(int64_t);
    int64_t acc = 0;
    for (size_t i = 0; i < ne; i++) {
        const StageItem &it = t.items[l->items[i]];
        first[i] = acc;
        acc += it.g.nblocks;
        const E e = make(it);
        memcpy(ent + i * sizeof(E), &e, sizeof e);
    }
    HIP_CHECK(hipMalloc(&l->d_mem, host.size()));
    HIP_CHECK(hipMemcpy(l->d_mem, host.data(), host.size(),
                        hipMemcpyHostToDevice));
    return 0;
}

static pa_status upload_stage(StageTable *t)
{
    for (auto &l : t->launches) {
        if (!l.grouped) continue;
        pa_status st;
        switch (t->items[l.items[0]].fam) {
        case FAM_FILL:
            st = upload_launch<GFill>(
                *t, &l, [](const StageItem &it) { return it.fs.g; });
            break;
        case FAM_SOA:
            st = upload_launch<GSoa>(*t, &l, [](const StageItem &it) {
                GSoa g;
                memset(&g, 0, sizeof g);
                g.d = to_dev(it.s.d);
                g.aos = it.aos;
                for (int c = 0; c < it.s.n && c < PA_SOA_TILE_MAX_N; c++)
                    g.f[c] = it.fields[c];
                g.ta = it.s.ta;
                g.ti = it.s.ti;
                g.pitch = it.s.pitch;
                g.plane = it.s.plane;
                g.ntile_i = it.g.nti;
                g.ntile_j = it.g.njc;
                return g;
            });
            break;
        default:
            st = upload_launch<GEntry>(*t, &l, [](const StageItem &it) {
                const bool copy = it.fam == FAM_COPY;
                GEntry g;
                memset(&g, 0, sizeof g);
                g.d = to_dev(copy ? it.k.d : it.c.d);
                g.src = it.src;
                g.dst = it.dst;
                g.ta = copy ? it.k.ta : it.c.ta;
                g.ntile_i = it.g.nti;
                g.njchunk = it.g.njc;
                return g;
            });
        }
        if (st) return st;
    }
    return 0;
}

/* One grouped launch.  `it` is its first entry: everything that picks the
 * kernel instance (the signature and, per family, the wire pair, the scalar
 * type, the counts, the split / join tile shape) is the same for all of them.
 * scalar and alpha as in launch_row(). */
static pa_status launch_group(const StageLaunch &l, const StageItem &it,
                              int scalar, double alpha, hipStream_t stream)
{
    const int ne = (int)l.items.size();
    const int64_t *first = (const int64_t *)l.d_mem;
    const void *table = (const char *)l.d_mem + ne * sizeof(int64_t);
    const GEntry *ent = (const GEntry *)table;
    const int64_t nb = l.nblocks;
    auto none = [](auto...) {
        return fail("kernel kind without a grouped form");
    };
    dim3 grid;
    pa_status st;
    switch (it.fam) {
    case FAM_FILL:
        if (pa_status gst = grid2d(nb, 256, &grid)) return gst;
        st = launch(k_group_fill, grid, dim3(256), 0, stream, first,
                    (const GFill *)table, ne, nb);
        break;
    case FAM_CVT:
        if (pa_status gst = cvt_dim(it.c.kind, nb, &grid)) return gst;
        st = for_cvt(
            it.c,
            [&](auto w, auto o, auto v) {
                return launch(k_group_cvt_linear<w, o, v>, grid, dim3(256), 0,
                              stream, first, ent, ne, nb);
            },
            [&](auto w, auto o, auto nc) {
                return launch(k_group_cvt_tile<w, o, nc>, grid, dim3(64, 16),
                              0, stream, first, ent, ne, nb);
            },
            none);
        break;
    case FAM_SCALE:
        if (pa_status gst = cvt_dim(it.c.kind, nb, &grid)) return gst;
        st = for_scale(
            it.c, alpha,
            [&](auto a, auto v) {
                return launch(k_group_scale_linear<decltype(a), v>, grid,
                              dim3(256), 0, stream, first, ent, ne, nb, a);
            },
            [&](auto a, auto nc) {
                return launch(k_group_scale_tile<decltype(a), nc>, grid,
                              dim3(64, 16), 0, stream, first, ent, ne, nb, a);
            },
            none);
        break;
    case FAM_SOA:
        if (pa_status gst = grid2d(nb, 256, &grid)) return gst;
        st = for_soa(
            it.s, scalar, alpha,
            [&](auto s, auto m, auto dir, auto n, auto v) {
                using S = typename decltype(s)::type;
                return launch(k_group_soa_linear<S, dir, n, v, decltype(m)>,
                              grid, dim3(256), 0, stream, first,
                              (const GSoa *)table, ne, nb, m);
            },
            [&](auto s, auto m, auto dir, auto n, size_t lds) {
                using S = typename decltype(s)::type;
                return launch(k_group_soa_tile<S, dir, n, decltype(m)>, grid,
                              dim3(64, 4), lds, stream, first,
                              (const GSoa *)table, ne, nb, m);
            },
            none);
        break;
    default: /* FAM_COPY: the signature holds the grouped kind and the word */
        st = for_word(l.sig.word, [&](auto tag) -> pa_status {
            using T = typename decltype(tag)::type;
            constexpr bool wide = sizeof(T) == 16;
            constexpr int NR = wide ? 8 : 16;
            switch (l.sig.kind) {
            case PA_KERNEL_LINEAR:
                if (pa_status gst = grid2d(nb, 256, &grid)) return gst;
                return launch(k_group_linear<T>, grid, dim3(256), 0, stream,
                              first, ent, ne, nb);
            case PA_KERNEL_TILE_VS:
                if constexpr (sizeof(T) == 8) {
                    if (pa_status gst = grid2d(nb, 64 * 16, &grid)) return gst;
                    return launch(k_group_tile_vs<T, 64, 128, 16>, grid,
                                  dim3(64, 16), 0, stream, first, ent, ne, nb);
                }
                break;
            case PA_KERNEL_TILE:
                if (pa_status gst = grid2d(nb, 64 * NR, &grid)) return gst;
                return launch(
                    k_group_tile<T, wide ? 32 : 128, wide ? 32 : 64, NR>,
                    grid, dim3(64, NR), 0, stream, first, ent, ne, nb);
            }
            return fail("bad grouped kind %d", l.sig.kind);
        });
    }
    if (st) return st;
    HIP_CHECK(hipGetLastError());
    return 0;
}

/* One row of a stage table, grouped or single, by its family.  alpha
 * multiplies in the scaling kernels; scalar is the PA_SCALAR_* code of a
 * scaling split / join call, 0 for a plain one. */
static pa_status launch_row(const StageTable &t, const StageLaunch &l,
                            int scalar, double alpha, hipStream_t stream)
{
    const StageItem &it = t.items[l.items[0]];
    if (l.grouped) return launch_group(l, it, scalar, alpha, stream);
    switch (it.fam) {
    case FAM_COPY:
        return launch_sel(it.k, it.src, it.dst, stream);
    case FAM_CVT:
        return launch_cvt_sel(it.c, it.src, it.dst, stream);
    case FAM_SCALE:
        return launch_scale_sel(it.c, it.src, it.dst, alpha, stream);
    case FAM_SOA:
        return launch_soa_sel(it.s, it.aos, it.fields.data(), scalar, alpha,
                              stream);
    default:
        return fail("a fill entry outside a grouped launch");
    }
}

static void stage_key(const pa_plan *p, int n, int stage,
                      const void *const *srcs, void *const *dsts,
                      std::vector<uintptr_t> *key)
{
    key->clear();
    key->push_back((uintptr_t)n);
    key->push_back((uintptr_t)stage);
    key->push_back((uintptr_t)p->send_buf);
    key->push_back((uintptr_t)p->recv_buf);
    for (int f = 0; f < n; f++) {
        key->push_back(stage != STAGE_UNPACK ? (uintptr_t)srcs[f] : 0);
        key->push_back(stage != STAGE_PACK ? (uintptr_t)dsts[f] : 0);
    }
}

static pa_status many_check(const pa_plan *p, int n, int stage,
                            const void *const *srcs, void *const *dsts)
{
    if (!p) return fail("null plan");
    if (n < 1) return fail("n must be >= 1 (got %d)", n);
    if (stage != STAGE_UNPACK) {
        if (!srcs) return fail("null srcs");
        for (int f = 0; f < n; f++)
            if (!srcs[f]) return fail("null src pointer for field %d", f);
    }
    if (stage != STAGE_PACK) {
        if (!dsts) return fail("null dsts");
        for (int f = 0; f < n; f++)
            if (!dsts[f]) return fail("null dst pointer for field %d", f);
    }
    if (p->own_bufs &&
        !((p->keep || pa_plan_group_cvt(p) || p->scale) && n == 1))
        return fail("multi-field stages need staging buffers of "
                    "pa_plan_buffer_sizes_many bytes from pa_plan_set_buffers");
    if ((p->send_total > 0 && !p->send_buf) ||
        (p->recv_total > 0 && !p->recv_buf))
        return fail("missing staging buffers: call pa_plan_set_buffers with "
                    "pa_plan_buffer_sizes_many bytes");
    return 0;
}

/* The single-group exchange of n fields: one message per peer at the
 * pa_plan_peer_message ranges, on the comm stream, ordered after the packs
 * already enqueued on `stream`; ev_comm is recorded behind it. */
static pa_status exchange_many(pa_plan *p, int n, hipStream_t stream)
{
    if (pa_status st = ensure_comm_stream(p)) return st;
    HIP_CHECK(hipEventRecord(p->ev_pack, stream));
    HIP_CHECK(hipStreamWaitEvent(p->comm_stream, p->ev_pack, 0));
    TM_REC(3, p->comm_stream);
    NCCL_CHECK(ncclGroupStart());
    for (auto &blk : p->peers) {
        if (blk.k == p->myk) continue;
        int64_t m[4];
        if (pa_status st = pa_plan_peer_message(p, n, blk.k, m)) return st;
        if (m[3])
            NCCL_CHECK(ncclRecv((char *)p->recv_buf + m[2], (size_t)m[3],
                                ncclUint8, blk.k, p->comm->comm,
                                p->comm_stream));
        if (m[1])
            NCCL_CHECK(ncclSend((const char *)p->send_buf + m[0],
                                (size_t)m[1], ncclUint8, blk.k,
                                p->comm->comm, p->comm_stream));
    }
    NCCL_CHECK(ncclGroupEnd());
    TM_REC(4, p->comm_stream);
    HIP_CHECK(hipEventRecord(p->ev_comm, p->comm_stream));
    return 0;
}

/* The second word of a table key says which stage the table is of: the
 * n-field stages carry their STAGE_* code (stage_key()), the split / join
 * stages STAGE_CODE_SOA + 4 * direction + stage, past all of those. */
enum { STAGE_CODE_SOA = 16 };

/* The plan's LRU cache of stage tables: the table of `key`, built by
 * build(table) and uploaded on a miss, after dropping the least recently
 * used one at capacity. */
template <typename Build>
static pa_status stage_table_get(pa_plan *p, const std::vector<uintptr_t> &key,
                                 StageTable **out, Build build)
{
    StageTable *t = nullptr;
    for (auto *c : p->tables)
        if (c->key == key) { t = c; break; }
    if (!t) {
        if ((int)p->tables.size() >= PA_STAGE_TABLES_MAX) {
            size_t old = 0;
            for (size_t i = 1; i < p->tables.size(); i++)
                if (p->tables[i]->stamp < p->tables[old]->stamp) old = i;
            free_table(p->tables[old]);
            p->tables.erase(p->tables.begin() + old);
        }
        t = new StageTable;
        t->key = key;
        pa_status st = build(t);
        if (!st) st = upload_stage(t);
        if (st) { free_table(t); return st; }
        p->tables.push_back(t);
        p->table_builds++;
    }
    t->stamp = ++p->table_clock;
    *out = t;
    return 0;
}

/* the (kind, grouped, entries, workgroups) rows the stage queries report */
static void table_rows(const StageTable &t, int max_rows, int64_t (*rows)[4],
                       int *nrows)
{
    *nrows = (int)t.launches.size();
    for (int i = 0; i < *nrows && i < max_rows; i++) {
        const StageLaunch &l = t.launches[i];
        rows[i][0] = l.sig.kind;
        rows[i][1] = l.grouped ? 1 : 0;
        rows[i][2] = (int64_t)l.items.size();
        rows[i][3] = l.nblocks;
    }
}

static pa_status run_table(const StageTable &t, int scalar, double alpha,
                           hipStream_t stream)
{
    for (auto &l : t.launches)
        if (pa_status st = launch_row(t, l, scalar, alpha, stream)) return st;
    return 0;
}

static pa_status run_stage(pa_plan *p, int n, int stage,
                           const void *const *srcs, void *const *dsts,
                           hipStream_t stream)
{
    if (pa_status st = many_check(p, n, stage, srcs, dsts)) return st;
    std::vector<uintptr_t> key;
    stage_key(p, n, stage, srcs, dsts, &key);
    StageTable *t;
    if (pa_status st = stage_table_get(p, key, &t, [&](StageTable *nt) {
            return build_stage(p, n, stage, srcs, dsts, p->send_buf,
                               p->recv_buf, nt);
        }))
        return st;
    return run_table(*t, 0, p->alpha, stream);
}

extern "C" {

pa_status pa_plan_buffer_sizes_many(const pa_plan *p, int n,
                                    int64_t *send_bytes, int64_t *recv_bytes)
{
    if (!p || !send_bytes || !recv_bytes) return fail("null argument");
    if (n < 1) return fail("n must be >= 1 (got %d)", n);
    *send_bytes = (int64_t)n * p->send_total * p->msg_esz;
    *recv_bytes = (int64_t)n * p->recv_total * p->msg_esz;
    return 0;
}

pa_status pa_plan_peer_message(const pa_plan *p, int n, int k, int64_t out[4])
{
    if (!p || !out) return fail("null argument");
    if (n < 1) return fail("n must be >= 1 (got %d)", n);
    if (p->R < 0 || k < 0 || k >= (int)p->peers.size())
        return fail("no peer block %d", k);
    const PeerBlockC &b = p->peers[k];
    if (k == p->myk) { /* the self block is never a message */
        out[0] = out[1] = out[2] = out[3] = 0;
        return 0;
    }
    out[0] = (int64_t)n * b.send_off * p->msg_esz;
    out[1] = (int64_t)n * b.send_n * p->msg_esz;
    out[2] = (int64_t)n * b.recv_off * p->msg_esz;
    out[3] = (int64_t)n * b.recv_n * p->msg_esz;
    return 0;
}

pa_status pa_plan_copydesc_many(const pa_plan *p, int n, int f, int which,
                                int k, int64_t *nd, int64_t *dims,
                                int64_t *sstr, int64_t *soff, int64_t *dstr,
                                int64_t *doff)
{
    if (!p) return fail("null plan");
    static const char *const staged[2] = {"block", "block"};
    if (p->keep) return keep_has_no_single();
    CopyDescH d;
    if (pa_status st = single_desc(p, n, f, which, k, staged, &d)) return st;
    copy_out(d, nd, dims, sstr, soff, dstr, doff);
    return 0;
}

pa_status pa_plan_stage_launches(const pa_plan *p, int n, int stage,
                                 const void *const *srcs, void *const *dsts,
                                 int max_rows, int64_t (*rows)[4], int *nrows)
{
    if (!p || !nrows) return fail("null argument");
    if (n < 1) return fail("n must be >= 1 (got %d)", n);
    if (stage < STAGE_PACK || stage > STAGE_UNPACK)
        return fail("bad stage %d", stage);
    /* staging as set, else assumed 256-byte aligned; never dereferenced */
    const void *send = p->send_buf ? p->send_buf : (const void *)256;
    void *recv = p->recv_buf ? p->recv_buf : (void *)256;
    std::vector<const void *> s(n, (const void *)256);
    std::vector<void *> d(n, (void *)256);
    for (int f = 0; f < n; f++) {
        if (srcs && srcs[f]) s[f] = srcs[f];
        if (dsts && dsts[f]) d[f] = dsts[f];
    }
    StageTable t;
    if (pa_status st =
            build_stage(p, n, stage, s.data(), d.data(), send, recv, &t))
        return st;
    table_rows(t, max_rows, rows, nrows);
    return 0;
}

int pa_plan_stage_table_count(const pa_plan *p)
{
    return p ? (int)p->tables.size() : 0;
}

int64_t pa_plan_stage_table_builds(const pa_plan *p)
{
    return p ? p->table_builds : 0;
}

/* ---- truncated transposes: introspection and the stand-alone fill ---- */

int pa_plan_nsub(const pa_plan *p, int which, int k)
{
    if (!p || !p->keep || which < 0 || which > 4) return 0;
    const std::vector<SubC> *l = block_list(p, which, k);
    return l ? (int)l->size() : 0;
}

pa_status pa_plan_copydesc_sub(const pa_plan *p, int n, int f, int which,
                               int k, int s, int64_t *nd, int64_t *dims,
                               int64_t *sstr, int64_t *soff, int64_t *dstr,
                               int64_t *doff)
{
    if (!p) return fail("null plan");
    if (!p->keep) return fail("not a keep plan");
    CopyDescH d;
    if (pa_status st = field_desc(p, n, f, which, k, s, &d)) return st;
    copy_out(d, nd, dims, sstr, soff, dstr, doff);
    return 0;
}

int pa_plan_nfill(const pa_plan *p)
{
    return p && p->keep ? (int)p->fills.size() : 0;
}

pa_status pa_plan_filldesc(const pa_plan *p, int i, int64_t *nd,
                           int64_t *dims, int64_t *dstr, int64_t *doff)
{
    if (!p || !p->keep) return fail("not a keep plan");
    if (i < 0 || i >= (int)p->fills.size()) return fail("no fill box %d", i);
    const FillDescH &d = p->fills[i];
    *nd = d.nd;
    for (int a = 0; a < d.nd; a++) {
        dims[a] = d.dims[a];
        dstr[a] = d.dstr[a];
    }
    *doff = d.doff;
    return 0;
}

static pa_status fill_args(int nd, const int64_t *dims, const int64_t *dstr,
                           int64_t doff, int64_t scalar_size, int64_t ncomp,
                           const void *dst, FillSel *out)
{
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    if (scalar_size <= 0 || ncomp <= 0) return fail("bad element size");
    for (int a = 0; a < nd; a++)
        if (dims[a] < 0 || dstr[a] < 0) return fail("bad fill window");
    FillDescH d = normalize_fill(nd, dims, dstr, doff);
    return select_fill(d, scalar_size * ncomp, dst, out);
}

pa_status pa_device_fill_zero(int nd, const int64_t *dims,
                              const int64_t *dstr, int64_t doff,
                              int64_t scalar_size, int64_t ncomp, void *dst,
                              void *stream)
{
    FillSel k;
    if (pa_status st =
            fill_args(nd, dims, dstr, doff, scalar_size, ncomp, dst, &k))
        return st;
    if (k.kind == PA_KERNEL_NONE) return 0; /* empty window: no launch */
    dim3 grid;
    if (pa_status st = grid2d(k.nblocks, 256, &grid)) return st;
    hipLaunchKernelGGL(k_fill, grid, dim3(256), 0, (hipStream_t)stream, k.g);
    HIP_CHECK(hipGetLastError());
    return 0;
}

pa_status pa_fill_kernel_kind(int nd, const int64_t *dims,
                              const int64_t *dstr, int64_t doff,
                              int64_t scalar_size, int64_t ncomp,
                              const void *dst, int64_t out[2])
{
    if (!out) return fail("null output");
    FillSel k;
    if (pa_status st =
            fill_args(nd, dims, dstr, doff, scalar_size, ncomp, dst, &k))
        return st;
    out[0] = k.kind;
    out[1] = k.kind == PA_KERNEL_NONE ? 0 : k.g.width;
    return 0;
}

pa_status pa_transpose_pack_many(pa_plan *p, int n, const void *const *srcs,
                                 void *stream)
{
    return run_stage(p, n, STAGE_PACK, srcs, nullptr, (hipStream_t)stream);
}

pa_status pa_transpose_local_many(pa_plan *p, int n, const void *const *srcs,
                                  void *const *dsts, void *stream)
{
    return run_stage(p, n, STAGE_LOCAL, srcs, dsts, (hipStream_t)stream);
}

pa_status pa_transpose_unpack_many(pa_plan *p, int n, void *const *dsts,
                                   void *stream)
{
    return run_stage(p, n, STAGE_UNPACK, nullptr, dsts, (hipStream_t)stream);
}

pa_status pa_transpose_execute_many(pa_plan *p, int n,
                                    const void *const *srcs,
                                    void *const *dsts, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (pa_status st = many_check(p, n, STAGE_LOCAL, srcs, dsts)) return st;

    const bool xchg = exchanging(p);
    if (xchg && !p->comm)
        return fail("subgroup exchange requires pa_plan_set_comm");
    if (pa_status st = timing_begin(p)) return st;

    /* 1. every pack and staged self pack of every field, before any write
     * of a destination */
    TM_REC(0, stream);
    if (pa_status st = run_stage(p, n, STAGE_PACK, srcs, nullptr, stream))
        return st;
    TM_REC(1, stream);

    /* 2. one grouped exchange, one message per peer carrying all n fields,
     * on the comm stream, event-ordered like pa_transpose_execute */
    if (xchg)
        if (pa_status st = exchange_many(p, n, stream)) return st;

    /* 3. fused local copies (aliased: staged self unpacks), overlapping the
     * exchange on the caller's stream */
    if (pa_status st = run_stage(p, n, STAGE_LOCAL, srcs, dsts, stream))
        return st;
    TM_REC(2, stream);

    /* 4. unpack every received block of every field */
    if (xchg) HIP_CHECK(hipStreamWaitEvent(stream, p->ev_comm, 0));
    TM_REC(5, stream);
    if (pa_status st = run_stage(p, n, STAGE_UNPACK, nullptr, dsts, stream))
        return st;
    TM_REC(6, stream);
    return 0;
}

} /* extern "C" */

/* ---- split and join transposes ----------------------------------------
 *
 * An ordinary scalar plan run with a vector-valued array on one side: n
 * scalars per element, components fastest.  The staging layout is the
 * multi-field one with the components as fields, so the opposite side's
 * stages are pa_transpose_*_many unchanged.  One launch per block, each
 * carrying all n components.  The *_scaled calls take a scale per call (a
 * plan with one set is refused) and launch the scaling form of the same
 * kernels: a split multiplies in pack and local, so its staging holds scaled
 * scalars; a join multiplies in local and unpack, so its staging does not. */

/* what a split or join call, and pa_plan_stage_launches_soa, refuse about
 * the plan and n */
static pa_status soa_check_plan(const pa_plan *p, int n)
{
    if (!p) return fail("null plan");
    if (n < 2) return fail("n must be >= 2 (got %d)", n);
    if (p->aliased)
        return fail("a split or join cannot run on a PA_PLAN_ALIASED plan: "
                    "the two sides have different element sizes and cannot "
                    "alias");
    if (p->keep && !pa_plan_group_soa(p))
        return fail("a split or join cannot run on a keep plan");
    if (p->wire) return fail("a split or join cannot run on a wire plan");
    if (p->scale)
        return fail("a split or join cannot run on a plan with a scale set");
    if (p->ncomp > 1)
        return fail("a split or join needs a scalar plan: this one has "
                    "ncomp = %lld", (long long)p->ncomp);
    return check_soa(p->ssz, n, PA_SOA_SPLIT);
}

static pa_status soa_check(const pa_plan *p, int n, const void *aos,
                           const void *const *fields, bool need_fields)
{
    if (pa_status st = soa_check_plan(p, n)) return st;
    if (!aos) return fail("null vector-valued array pointer");
    if (need_fields) {
        if (!fields) return fail("null field pointers");
        for (int c = 0; c < n; c++)
            if (!fields[c]) return fail("null pointer for field %d", c);
    }
    if (p->own_bufs)
        return fail("split and join stages need staging buffers of "
                    "pa_plan_buffer_sizes_many bytes from pa_plan_set_buffers");
    if ((p->send_total > 0 && !p->send_buf) ||
        (p->recv_total > 0 && !p->recv_buf))
        return fail("missing staging buffers: call pa_plan_set_buffers with "
                    "pa_plan_buffer_sizes_many bytes");
    return 0;
}

/* one staged block with the vector-valued array on its other side: component
 * c's slot starts c * (block count) scalars into the block */
static pa_status soa_staged(const pa_plan *p, int n, int dir, const SubC &sb,
                            void *aos, void *staging, int scale, double alpha,
                            hipStream_t stream)
{
    CopyDescH d = sb.d;
    const int64_t sh = many_shift(n, 0, sb.off, sb.n);
    if (dir == PA_SOA_SPLIT)
        d.doff += sh;
    else
        d.soff += sh;
    void *few[PA_SOA_GENERIC_PTRS];
    std::vector<void *> many;
    void **slots = few;
    if (n > PA_SOA_GENERIC_PTRS) {
        many.resize(n);
        slots = many.data();
    }
    for (int c = 0; c < n; c++)
        slots[c] = (char *)staging + (int64_t)c * sb.n * p->ssz;
    return launch_desc_soa(d, p->ssz, n, dir, aos, slots, stream, scale,
                           alpha);
}

/* The scale of a *_scaled stage call, checked after soa_check() and before
 * any pointer is touched: *scale is the PA_SCALAR_* code the launches get, 0
 * for alpha == 1, which runs exactly the plain call's code. */
static pa_status soa_scale(const pa_plan *p, int scalar, double alpha,
                           int *scale)
{
    if (pa_status st = check_soa_scale(p->ssz, scalar, alpha)) return st;
    *scale = alpha == 1.0 ? 0 : scalar;
    return 0;
}

/* ---- stage tables of the split / join stages (PA_PLAN_GROUP_SOA) -------
 *
 * The launch list of (dir, stage): select_kernel_soa() per sub-block in the
 * order the ungrouped stage loops walk them.  With `grouped` the SOA_LINEAR
 * entries of one V share a launch and so do all SOA_TILE entries (their tile
 * shape depends on n * S only), in first-appearance order; SOA_GENERIC
 * entries stay one row each.  The local stage of a keep plan ends with ONE
 * grouped PA_KERNEL_FILL row: the plan's fill windows on every field of a
 * split, and on the vector-valued array, in elements of n * S bytes, of a
 * join.  Host-only; staging may be any aligned stand-in. */
static pa_status build_stage_soa(const pa_plan *p, int n, int dir, int stage,
                                 void *aos, void *const *fields,
                                 void *send_buf, void *recv_buf, bool grouped,
                                 StageTable *t)
{
    auto add_desc = [&](const CopyDescH &d, void *const *fp) -> pa_status {
        StageItem it;
        it.fam = FAM_SOA;
        it.aos = aos;
        it.fields.assign(fp, fp + n);
        if (pa_status st = select_kernel_soa(d, p->ssz, n, dir, aos, fp, &it.s))
            return st;
        const SoaSel &k = it.s;
        it.g = soa_grid(k);
        StageSig sig;
        sig.kind = k.kind;
        sig.vec = k.kind == PA_KERNEL_SOA_LINEAR ? k.V : 0;
        stage_push(t, it, sig, grouped && k.kind != PA_KERNEL_SOA_GENERIC);
        return 0;
    };
    /* one staged block with the vector-valued array on its other side:
     * component c's slot starts c * (block count) scalars into the block */
    auto add_staged = [&](const SubC &sb, void *staging) -> pa_status {
        CopyDescH d = sb.d;
        const int64_t sh = many_shift(n, 0, sb.off, sb.n);
        if (dir == PA_SOA_SPLIT)
            d.doff += sh;
        else
            d.soff += sh;
        std::vector<void *> slots(n);
        for (int c = 0; c < n; c++)
            slots[c] = (char *)staging + (int64_t)c * sb.n * p->ssz;
        return add_desc(d, slots.data());
    };

    if (stage == STAGE_LOCAL) {
        for (auto &sb : p->local)
            if (pa_status st = add_desc(sb.d, fields)) return st;
        for (int c = 0; c < (dir == PA_SOA_SPLIT ? n : 1); c++)
            for (auto &fd : p->fills)
                if (pa_status st =
                        dir == PA_SOA_SPLIT
                            ? stage_add_fill(t, fd, p->ssz, fields[c])
                            : stage_add_fill(t, fd, (int64_t)n * p->ssz, aos))
                    return st;
        return 0;
    }
    for (auto &b : p->peers)
        for (auto &sb : dir == PA_SOA_SPLIT ? b.pack : b.unpack)
            if (pa_status st = add_staged(
                    sb, dir == PA_SOA_SPLIT ? send_buf : recv_buf))
                return st;
    return 0;
}

/* One split / join stage of a PA_PLAN_GROUP_SOA plan through its cached
 * table.  The key is (n, direction and stage, the vector-valued array, the
 * field pointers); neither the scale nor alpha is part of it, so a scaled
 * call, a plain one and one with another alpha share a table. */
static pa_status run_stage_soa(pa_plan *p, int n, int dir, int stage,
                               void *aos, void *const *fields, int scale,
                               double alpha, hipStream_t stream)
{
    std::vector<uintptr_t> key;
    key.push_back((uintptr_t)n);
    key.push_back((uintptr_t)(STAGE_CODE_SOA + 4 * dir + stage));
    key.push_back((uintptr_t)p->send_buf);
    key.push_back((uintptr_t)p->recv_buf);
    key.push_back((uintptr_t)aos);
    for (int c = 0; c < n; c++)
        key.push_back(stage == STAGE_LOCAL ? (uintptr_t)fields[c] : 0);
    StageTable *t;
    if (pa_status st = stage_table_get(p, key, &t, [&](StageTable *nt) {
            return build_stage_soa(p, n, dir, stage, aos, fields, p->send_buf,
                                   p->recv_buf, true, nt);
        }))
        return st;
    return run_table(*t, scale, alpha, stream);
}

/* The four stages behind the plain and the scaled calls, arguments already
 * checked; scale as soa_scale() returns it (0: none).  A PA_PLAN_GROUP_SOA
 * plan runs them through its stage tables. */
static pa_status soa_pack_split(pa_plan *p, int n, const void *src_aos,
                                int scale, double alpha, hipStream_t stream)
{
    if (pa_plan_group_soa(p))
        return run_stage_soa(p, n, PA_SOA_SPLIT, STAGE_PACK, (void *)src_aos,
                             nullptr, scale, alpha, stream);
    for (auto &b : p->peers)
        for (auto &sb : b.pack)
            if (pa_status st =
                    soa_staged(p, n, PA_SOA_SPLIT, sb, (void *)src_aos,
                               p->send_buf, scale, alpha, stream))
                return st;
    return 0;
}

static pa_status soa_local(pa_plan *p, int n, int dir, void *aos,
                           void *const *fields, int scale, double alpha,
                           hipStream_t stream)
{
    if (pa_plan_group_soa(p))
        return run_stage_soa(p, n, dir, STAGE_LOCAL, aos, fields, scale,
                             alpha, stream);
    for (auto &sb : p->local)
        if (pa_status st = launch_desc_soa(sb.d, p->ssz, n, dir, aos, fields,
                                           stream, scale, alpha))
            return st;
    return 0;
}

static pa_status soa_unpack_join(pa_plan *p, int n, void *dst_aos, int scale,
                                 double alpha, hipStream_t stream)
{
    if (pa_plan_group_soa(p))
        return run_stage_soa(p, n, PA_SOA_JOIN, STAGE_UNPACK, dst_aos,
                             nullptr, scale, alpha, stream);
    for (auto &b : p->peers)
        for (auto &sb : b.unpack)
            if (pa_status st = soa_staged(p, n, PA_SOA_JOIN, sb, dst_aos,
                                          p->recv_buf, scale, alpha, stream))
                return st;
    return 0;
}

extern "C" {

pa_status pa_device_copy_soa(int nd, const int64_t *dims, const int64_t *sstr,
                             int64_t soff, const int64_t *dstr, int64_t doff,
                             int64_t scalar_size, int n, int dir, void *aos,
                             void *const *fields, void *stream)
{
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    if (pa_status st = check_soa(scalar_size, n, dir)) return st;
    if (!aos || !fields) return fail("null pointer");
    for (int c = 0; c < n; c++)
        if (!fields[c]) return fail("null pointer for field %d", c);
    CopyDescH d = normalize_desc(nd, dims, sstr, soff, dstr, doff);
    return launch_desc_soa(d, scalar_size, n, dir, aos, fields,
                           (hipStream_t)stream);
}

pa_status pa_device_copy_soa_scale(int nd, const int64_t *dims,
                                   const int64_t *sstr, int64_t soff,
                                   const int64_t *dstr, int64_t doff,
                                   int64_t scalar_size, int n, int dir,
                                   int scalar, double alpha, void *aos,
                                   void *const *fields, void *stream)
{
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    if (pa_status st = check_soa(scalar_size, n, dir)) return st;
    if (pa_status st = check_soa_scale(scalar_size, scalar, alpha)) return st;
    if (!aos || !fields) return fail("null pointer");
    for (int c = 0; c < n; c++)
        if (!fields[c]) return fail("null pointer for field %d", c);
    CopyDescH d = normalize_desc(nd, dims, sstr, soff, dstr, doff);
    /* always the scaling kernel, alpha == 1 included */
    return launch_desc_soa(d, scalar_size, n, dir, aos, fields,
                           (hipStream_t)stream, scalar, alpha);
}

pa_status pa_copy_kernel_kind_soa(int nd, const int64_t *dims,
                                  const int64_t *sstr, int64_t soff,
                                  const int64_t *dstr, int64_t doff,
                                  int64_t scalar_size, int n, int dir,
                                  const void *aos, const void *const *fields,
                                  int64_t out[5])
{
    if (!out) return fail("null output");
    if (nd <= 0 || nd > MAXND) return fail("bad nd");
    if (pa_status st = check_soa(scalar_size, n, dir)) return st;
    CopyDescH d = normalize_desc(nd, dims, sstr, soff, dstr, doff);
    SoaSel k;
    if (pa_status st =
            select_kernel_soa(d, scalar_size, n, dir, aos, fields, &k))
        return st;
    out[0] = k.kind;
    out[1] = k.V;
    out[2] = k.ti;
    out[3] = k.tj;
    out[4] = 1; /* the split/join tile sweeps one tile per workgroup */
    return 0;
}

pa_status pa_plan_stage_launches_soa(const pa_plan *p, int n, int dir,
                                     int stage, const void *aos,
                                     const void *const *fields, int max_rows,
                                     int64_t (*rows)[4], int *nrows)
{
    if (!nrows || (max_rows > 0 && !rows)) return fail("null argument");
    if (pa_status st = soa_check_plan(p, n)) return st;
    if (dir != PA_SOA_SPLIT && dir != PA_SOA_JOIN)
        return fail("unknown direction %d: PA_SOA_SPLIT or PA_SOA_JOIN", dir);
    if (stage < STAGE_PACK || stage > STAGE_UNPACK)
        return fail("bad stage %d", stage);
    if (stage == (dir == PA_SOA_SPLIT ? STAGE_UNPACK : STAGE_PACK))
        return fail("the %s of a %s is the ordinary n-field stage: ask "
                    "pa_plan_stage_launches",
                    dir == PA_SOA_SPLIT ? "unpack" : "pack",
                    dir == PA_SOA_SPLIT ? "split" : "join");
    /* staging as set, else assumed 256-byte aligned, like absent pointers;
     * never dereferenced */
    void *send = p->send_buf ? p->send_buf : (void *)256;
    void *recv = p->recv_buf ? p->recv_buf : (void *)256;
    std::vector<void *> f(n, (void *)256);
    for (int c = 0; fields && c < n; c++)
        if (fields[c]) f[c] = (void *)fields[c];
    StageTable t;
    if (pa_status st = build_stage_soa(p, n, dir, stage,
                                       aos ? (void *)aos : (void *)256,
                                       f.data(), send, recv,
                                       pa_plan_group_soa(p) != 0, &t))
        return st;
    table_rows(t, max_rows, rows, nrows);
    return 0;
}

pa_status pa_transpose_pack_split(pa_plan *p, int n, const void *src_aos,
                                  void *stream)
{
    if (pa_status st = soa_check(p, n, src_aos, nullptr, false)) return st;
    return soa_pack_split(p, n, src_aos, 0, 1.0, (hipStream_t)stream);
}

pa_status pa_transpose_local_split(pa_plan *p, int n, const void *src_aos,
                                   void *const *dsts, void *stream)
{
    if (pa_status st = soa_check(p, n, src_aos, dsts, true)) return st;
    return soa_local(p, n, PA_SOA_SPLIT, (void *)src_aos, dsts, 0, 1.0,
                     (hipStream_t)stream);
}

pa_status pa_transpose_local_join(pa_plan *p, int n, const void *const *srcs,
                                  void *dst_aos, void *stream)
{
    if (pa_status st = soa_check(p, n, dst_aos, srcs, true)) return st;
    return soa_local(p, n, PA_SOA_JOIN, dst_aos, (void *const *)srcs, 0, 1.0,
                     (hipStream_t)stream);
}

pa_status pa_transpose_unpack_join(pa_plan *p, int n, void *dst_aos,
                                   void *stream)
{
    if (pa_status st = soa_check(p, n, dst_aos, nullptr, false)) return st;
    return soa_unpack_join(p, n, dst_aos, 0, 1.0, (hipStream_t)stream);
}

pa_status pa_transpose_pack_split_scaled(pa_plan *p, int n, int scalar,
                                         double alpha, const void *src_aos,
                                         void *stream)
{
    int scale;
    if (pa_status st = soa_check(p, n, src_aos, nullptr, false)) return st;
    if (pa_status st = soa_scale(p, scalar, alpha, &scale)) return st;
    return soa_pack_split(p, n, src_aos, scale, alpha, (hipStream_t)stream);
}

pa_status pa_transpose_local_split_scaled(pa_plan *p, int n, int scalar,
                                          double alpha, const void *src_aos,
                                          void *const *dsts, void *stream)
{
    int scale;
    if (pa_status st = soa_check(p, n, src_aos, dsts, true)) return st;
    if (pa_status st = soa_scale(p, scalar, alpha, &scale)) return st;
    return soa_local(p, n, PA_SOA_SPLIT, (void *)src_aos, dsts, scale, alpha,
                     (hipStream_t)stream);
}

pa_status pa_transpose_local_join_scaled(pa_plan *p, int n, int scalar,
                                         double alpha,
                                         const void *const *srcs,
                                         void *dst_aos, void *stream)
{
    int scale;
    if (pa_status st = soa_check(p, n, dst_aos, srcs, true)) return st;
    if (pa_status st = soa_scale(p, scalar, alpha, &scale)) return st;
    return soa_local(p, n, PA_SOA_JOIN, dst_aos, (void *const *)srcs, scale,
                     alpha, (hipStream_t)stream);
}

pa_status pa_transpose_unpack_join_scaled(pa_plan *p, int n, int scalar,
                                          double alpha, void *dst_aos,
                                          void *stream)
{
    int scale;
    if (pa_status st = soa_check(p, n, dst_aos, nullptr, false)) return st;
    if (pa_status st = soa_scale(p, scalar, alpha, &scale)) return st;
    return soa_unpack_join(p, n, dst_aos, scale, alpha, (hipStream_t)stream);
}

/* the hop shared by both: pack, the single-group exchange of
 * pa_transpose_execute_many, local, unpack; exactly one of src_aos / dst_aos
 * is set.  scaled: a *_scaled call, whose scalar and alpha are checked here;
 * a split multiplies in pack and local, a join in local and unpack. */
static pa_status execute_soa(pa_plan *p, int n, const void *src_aos,
                             const void *const *srcs, void *dst_aos,
                             void *const *dsts, bool scaled, int scalar,
                             double alpha, hipStream_t stream)
{
    const bool split = src_aos != nullptr;
    if (pa_status st = soa_check(p, n, split ? src_aos : dst_aos,
                                 split ? (const void *const *)dsts : srcs,
                                 true))
        return st;
    int scale = 0;
    if (scaled)
        if (pa_status st = soa_scale(p, scalar, alpha, &scale)) return st;
    const bool xchg = exchanging(p);
    if (xchg && !p->comm)
        return fail("subgroup exchange requires pa_plan_set_comm");
    if (pa_status st = timing_begin(p)) return st;

    TM_REC(0, stream);
    if (pa_status st =
            split ? soa_pack_split(p, n, src_aos, scale, alpha, stream)
                  : pa_transpose_pack_many(p, n, srcs, stream))
        return st;
    TM_REC(1, stream);

    if (xchg)
        if (pa_status st = exchange_many(p, n, stream)) return st;

    if (pa_status st =
            split ? soa_local(p, n, PA_SOA_SPLIT, (void *)src_aos, dsts,
                              scale, alpha, stream)
                  : soa_local(p, n, PA_SOA_JOIN, dst_aos,
                              (void *const *)srcs, scale, alpha, stream))
        return st;
    TM_REC(2, stream);

    if (xchg) HIP_CHECK(hipStreamWaitEvent(stream, p->ev_comm, 0));
    TM_REC(5, stream);
    if (pa_status st =
            split ? pa_transpose_unpack_many(p, n, dsts, stream)
                  : soa_unpack_join(p, n, dst_aos, scale, alpha, stream))
        return st;
    TM_REC(6, stream);
#undef TM_REC
    return 0;
}

pa_status pa_transpose_execute_split(pa_plan *p, int n, const void *src_aos,
                                     void *const *dsts, void *stream)
{
    if (!src_aos) return fail("null vector-valued array pointer");
    return execute_soa(p, n, src_aos, nullptr, nullptr, dsts, false, 0, 1.0,
                       (hipStream_t)stream);
}

pa_status pa_transpose_execute_join(pa_plan *p, int n,
                                    const void *const *srcs, void *dst_aos,
                                    void *stream)
{
    if (!dst_aos) return fail("null vector-valued array pointer");
    return execute_soa(p, n, nullptr, srcs, dst_aos, nullptr, false, 0, 1.0,
                       (hipStream_t)stream);
}

pa_status pa_transpose_execute_split_scaled(pa_plan *p, int n, int scalar,
                                            double alpha,
                                            const void *src_aos,
                                            void *const *dsts, void *stream)
{
    if (!src_aos) return fail("null vector-valued array pointer");
    return execute_soa(p, n, src_aos, nullptr, nullptr, dsts, true, scalar,
                       alpha, (hipStream_t)stream);
}

pa_status pa_transpose_execute_join_scaled(pa_plan *p, int n, int scalar,
                                           double alpha,
                                           const void *const *srcs,
                                           void *dst_aos, void *stream)
{
    if (!dst_aos) return fail("null vector-valued array pointer");
    return execute_soa(p, n, nullptr, srcs, dst_aos, nullptr, true, scalar,
                       alpha, (hipStream_t)stream);
}

} /* extern "C" */
