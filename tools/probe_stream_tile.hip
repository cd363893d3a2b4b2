/* probe_stream_tile.hip — cache-policy probe for the 8-byte vector-store
 * transpose tile (k_transpose_tile_vs<u64,64,128,16,JC>).
 *
 * The headline (1024^3 f64 permuted x->y) is one launch of that tile at
 * ~5.6-5.7 TB/s against 6.5 TB/s for a 1-D copy of the same bytes; the
 * direction probes put the gap on the write side (profiles/
 * r01_pattern_ceilings.txt, r2_kernel_stats.md).  Plain, sc0 and nt stores
 * all park the line in the XCD's L2 and leave in replacement order; sc1
 * stores write through and drop the line.  This probe measures, on the
 * shipped tile and with nothing else changed:
 *
 *   store policy  plain | nt | sc1 | sc0 sc1      (16-B vector stores only;
 *                                                  tail stores stay plain)
 *   load policy   plain | nt | sc1                (input read exactly once)
 *   sweep order   contiguous (workgroup c sweeps j-tiles JC*c .. JC*c+JC-1)
 *                 strided    (workgroup c sweeps c, c+njc, c+2*njc, ...)
 *
 * Stages:
 *   CHECK  every variant at every sweep depth on an odd shape (partial
 *          i-tile, short last chunk, odd j tail, padded pitch), the whole
 *          0xAB-prefilled destination compared byte for byte with a host
 *          transpose of the same seeded input;
 *   TRUE   all 24 variants interleaved round by round at 1024 x 2^20
 *          (8 MiB output pitch), median and min..max;
 *   WPAT   the one-direction write-pattern ceiling of the tile's store
 *          phase under each store policy, plus a contiguous 1-D write;
 *   SIZE   control, the best store-only variant and the overall winner at
 *          128 MiB .. 8 GiB payloads, with the production sweep-depth rule.
 *
 * GB/s = 2 * payload / time / 1e9 (WPAT: 1 * payload).
 *
 * Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 probe_stream_tile.hip \
 *            -o probe_stream_tile
 * Run:   ./probe_stream_tile [rounds]        (default 24)
 */

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHK(x)                                                               \
    do {                                                                     \
        hipError_t e_ = (x);                                                 \
        if (e_ != hipSuccess) {                                              \
            fprintf(stderr, "HIP error %s at %d\n", hipGetErrorName(e_),     \
                    __LINE__);                                               \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

enum { ST_PLAIN = 0, ST_NT = 1, ST_SC1 = 2, ST_SC0SC1 = 3, N_ST = 4 };
enum { LD_PLAIN = 0, LD_NT = 1, LD_SC1 = 2, N_LD = 3 };
static const char *ST_NAME[N_ST] = {"plain", "nt", "sc1", "sc0sc1"};
static const char *LD_NAME[N_LD] = {"plain", "nt", "sc1"};
static const char *SW_NAME[2] = {"contig", "strided"};

/* 16-B vector store with the chosen cache bits.  The asm forms end in
 * s_nop 1: a >8-B store reads its data registers one state late, and the
 * compiler does not pad after an asm statement. */
template <int ST>
__device__ __forceinline__ void store16(uint64_t *p, v4u q)
{
    if (ST == ST_PLAIN)
        *(v4u *)p = q;
    else if (ST == ST_NT)
        asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1"
                     :: "v"(p), "v"(q) : "memory");
    else if (ST == ST_SC1)
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1"
                     :: "v"(p), "v"(q) : "memory");
    else
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1"
                     :: "v"(p), "v"(q) : "memory");
}

template <int LD>
__device__ __forceinline__ uint64_t load8(const uint64_t *p)
{
    if (LD == LD_NT) return __builtin_nontemporal_load(p);
    if (LD == LD_SC1) /* relaxed agent-scope load = global_load ... sc1 */
        return __hip_atomic_load(p, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}

/* the shipped tile_vs_body at nd = 2: src[i + NI*j] -> dst[j + pitch*i] */
template <int JC, int ST, int LD, int SW>
__global__ __launch_bounds__(64 * 16) void t_vs(
    const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, int64_t NI,
    int64_t NJ, int64_t pitch, int64_t ntile_i, int64_t njchunk)
{
    constexpr int TI = 64, TJ = 128, NROWS = 16;
    __shared__ uint64_t tile[TI][TJ + 2];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int64_t bid = blockIdx.x;
    const int64_t t_i = bid % ntile_i;
    const int64_t chunk = bid / ntile_i;
    const int64_t i0 = t_i * TI;
    const int64_t ni = NI - i0 < TI ? NI - i0 : TI;

    for (int jt = 0; jt < JC; jt++) {
        const int64_t j0 =
            (SW ? chunk + jt * njchunk : chunk * JC + jt) * TJ;
        if (j0 >= NJ) break;
        const int64_t nj = NJ - j0 < TJ ? NJ - j0 : TJ;
        {
            const int64_t base = i0 + j0 * NI;
            for (int j = ty; j < nj; j += NROWS) {
                const int64_t row = base + (int64_t)j * NI;
                for (int i = tx; i < ni; i += 64)
                    tile[i][j] = load8<LD>(&src[row + i]);
            }
        }
        __syncthreads();
        {
            const int64_t base = j0 + i0 * pitch;
            const int64_t njv = nj & ~(int64_t)1;
            for (int i = ty; i < ni; i += NROWS) {
                uint64_t *row = dst + base + (int64_t)i * pitch;
                for (int j2 = 2 * tx; j2 < njv; j2 += 128) {
                    v4u q;
                    ((uint64_t *)&q)[0] = tile[i][j2];
                    ((uint64_t *)&q)[1] = tile[i][j2 + 1];
                    store16<ST>(&row[j2], q);
                }
                if ((nj & 1) && tx == 0) row[nj - 1] = tile[i][nj - 1];
            }
        }
        __syncthreads();
    }
}

/* the tile's store phase alone (full tiles only): 64 rows x 128 j per tile,
 * 16 row-threads, contiguous sweep */
template <int JC, int ST>
__global__ __launch_bounds__(64 * 16) void w_vs(uint64_t *__restrict__ dst,
                                                int64_t pitch,
                                                int64_t ntile_i)
{
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int64_t t_i = (int64_t)blockIdx.x % ntile_i;
    const int64_t chunk = (int64_t)blockIdx.x / ntile_i;
    for (int jt = 0; jt < JC; jt++) {
        const int64_t j0 = (chunk * JC + jt) * 128;
        for (int i = ty; i < 64; i += 16) {
            uint64_t *row = dst + j0 + (t_i * 64 + i) * pitch;
            v4u q = {(unsigned)tx, (unsigned)i, (unsigned)jt, (unsigned)j0};
            store16<ST>(&row[2 * tx], q);
        }
    }
}

/* contiguous 1-D write, 16 B per lane */
__global__ __launch_bounds__(256) void w_1d(v4u *__restrict__ dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (v4u){(unsigned)i, 1u, 2u, 3u};
}

__host__ __device__ static inline uint64_t mix(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull; /* splitmix64 of (index + seed) */
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
#define SEED 0xC0FFEEull

__global__ __launch_bounds__(256) void k_fill(uint64_t *p, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n; i += stride) p[i] = mix((uint64_t)i + SEED);
}

typedef void (*launch_fn)(const uint64_t *, uint64_t *, int64_t, int64_t,
                          int64_t);

template <int JC, int ST, int LD, int SW>
static void launch_t(const uint64_t *s, uint64_t *d, int64_t NI, int64_t NJ,
                     int64_t pitch)
{
    const int64_t nti = (NI + 63) / 64, ntj = (NJ + 127) / 128;
    const int64_t njc = (ntj + JC - 1) / JC;
    hipLaunchKernelGGL((t_vs<JC, ST, LD, SW>), dim3((uint32_t)(nti * njc)),
                       dim3(64, 16), 0, 0, s, d, NI, NJ, pitch, nti, njc);
}

#define ROW_SW(JC, ST, LD) {launch_t<JC, ST, LD, 0>, launch_t<JC, ST, LD, 1>}
#define ROW_LD(JC, ST) {ROW_SW(JC, ST, 0), ROW_SW(JC, ST, 1), ROW_SW(JC, ST, 2)}
#define ROW_ST(JC) {ROW_LD(JC, 0), ROW_LD(JC, 1), ROW_LD(JC, 2), ROW_LD(JC, 3)}
static const int JCS[3] = {1, 8, 32};
static launch_fn TAB[3][N_ST][N_LD][2] = {ROW_ST(1), ROW_ST(8), ROW_ST(32)};

/* the production sweep-depth rule (sweep_depth() in pencilhip.hip) */
static int depth_index(int64_t NI, int64_t NJ)
{
    const int64_t nti = (NI + 63) / 64, ntj = (NJ + 127) / 128;
    if (ntj * nti >= 32 * 4096 && ntj >= 256) return 2;
    if (ntj * nti >= 8 * 4096 && ntj >= 64) return 1;
    return 0;
}

struct Stat { double med, lo, hi; };
static Stat stat_of(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    return {n % 2 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]), v.front(),
            v.back()};
}

static hipEvent_t ev_a, ev_b;
template <class F> static double time_ms(F &&f, int reps)
{
    float ms;
    CHK(hipEventRecord(ev_a));
    for (int r = 0; r < reps; r++) f();
    CHK(hipEventRecord(ev_b));
    CHK(hipEventSynchronize(ev_b));
    CHK(hipEventElapsedTime(&ms, ev_a, ev_b));
    return ms / reps;
}

/* one table row: GB/s median and min..max (max time = min rate) */
static void row(const char *stage, const char *name, const char *size,
                double bytes, const Stat &t)
{
    printf("%-5s %-30s %-9s median %7.1f  min..max %7.1f..%7.1f GB/s  "
           "(%.4f ms)\n", stage, name, size, bytes / (t.med * 1e-3) / 1e9,
           bytes / (t.hi * 1e-3) / 1e9, bytes / (t.lo * 1e-3) / 1e9, t.med);
    fflush(stdout);
}

int main(int argc, char **argv)
{
    const int ROUNDS = argc > 1 ? atoi(argv[1]) : 24;
    if (ROUNDS < 1) return 2;
    const int64_t NIr = 1024, NJr = 1 << 20;
    const int64_t rbytes = NIr * NJr * 8;
    uint64_t *s, *d;
    CHK(hipMalloc((void **)&s, rbytes));
    CHK(hipMalloc((void **)&d, rbytes));
    CHK(hipEventCreate(&ev_a));
    CHK(hipEventCreate(&ev_b));
    hipLaunchKernelGGL(k_fill, dim3(65536), dim3(256), 0, 0, s, NIr * NJr);
    CHK(hipDeviceSynchronize());

    /* ---- CHECK: byte-for-byte against a host transpose ------------------ */
    int64_t nbad_total = 0;
    {
        const int64_t ni = 200, nj = 128 * 70 + 37, pitch = nj + 3;
        const int64_t dn = ni * pitch; /* whole destination, slack included */
        std::vector<uint64_t> exp((size_t)dn), got((size_t)dn);
        memset(exp.data(), 0xAB, (size_t)dn * 8);
        for (int64_t j = 0; j < nj; j++)
            for (int64_t i = 0; i < ni; i++)
                exp[(size_t)(j + pitch * i)] = mix((uint64_t)(i + ni * j) + SEED);
        for (int jc = 0; jc < 3; jc++)
            for (int st = 0; st < N_ST; st++)
                for (int ld = 0; ld < N_LD; ld++)
                    for (int sw = 0; sw < 2; sw++) {
                        CHK(hipMemset(d, 0xAB, (size_t)dn * 8));
                        TAB[jc][st][ld][sw](s, d, ni, nj, pitch);
                        CHK(hipGetLastError());
                        CHK(hipDeviceSynchronize());
                        CHK(hipMemcpy(got.data(), d, (size_t)dn * 8,
                                      hipMemcpyDeviceToHost));
                        int64_t bad = 0;
                        for (int64_t k = 0; k < dn; k++)
                            bad += got[(size_t)k] != exp[(size_t)k];
                        nbad_total += bad;
                        if (bad)
                            printf("CHECK c%-2d st=%s ld=%s %s FAIL (%lld "
                                   "bad)\n", JCS[jc], ST_NAME[st],
                                   LD_NAME[ld], SW_NAME[sw], (long long)bad);
                    }
        printf("CHECK 72 variants (3 depths x 4 store x 3 load x 2 sweep) at "
               "%lld x %lld pitch %lld: %s\n", (long long)ni, (long long)nj,
               (long long)pitch, nbad_total ? "FAIL" : "all byte-identical");
        fflush(stdout);
        if (nbad_total) return 1;
    }

    /* ---- TRUE: all variants interleaved at 1024 x 2^20 ------------------ */
    const double rio = 2.0 * rbytes;
    int best_st = 0, win_st = 0, win_ld = 0, win_sw = 0;
    {
        std::vector<double> t[N_ST][N_LD][2];
        for (int st = 0; st < N_ST; st++) /* warm every code object */
            for (int ld = 0; ld < N_LD; ld++)
                for (int sw = 0; sw < 2; sw++)
                    TAB[2][st][ld][sw](s, d, NIr, NJr, NJr);
        CHK(hipDeviceSynchronize());
        for (int r = 0; r < ROUNDS; r++)
            for (int st = 0; st < N_ST; st++)
                for (int ld = 0; ld < N_LD; ld++)
                    for (int sw = 0; sw < 2; sw++)
                        t[st][ld][sw].push_back(time_ms(
                            [&] { TAB[2][st][ld][sw](s, d, NIr, NJr, NJr); },
                            1));
        double best_store = 1e30, best_all = 1e30;
        for (int st = 0; st < N_ST; st++)
            for (int ld = 0; ld < N_LD; ld++)
                for (int sw = 0; sw < 2; sw++) {
                    char nm[64];
                    snprintf(nm, sizeof nm, "st=%s ld=%s %s", ST_NAME[st],
                             LD_NAME[ld], SW_NAME[sw]);
                    const Stat q = stat_of(t[st][ld][sw]);
                    row("TRUE", nm, "8GiB", rio, q);
                    if (ld == 0 && sw == 0 && q.med < best_store) {
                        best_store = q.med;
                        best_st = st;
                    }
                    if (q.med < best_all) {
                        best_all = q.med;
                        win_st = st, win_ld = ld, win_sw = sw;
                    }
                }
        printf("TRUE  best store-only: st=%s; overall winner: st=%s ld=%s "
               "%s\n", ST_NAME[best_st], ST_NAME[win_st], LD_NAME[win_ld],
               SW_NAME[win_sw]);

        /* the winner's output at the true shape: three whole 8 MiB rows */
        CHK(hipMemset(d, 0xAB, rbytes));
        TAB[2][win_st][win_ld][win_sw](s, d, NIr, NJr, NJr);
        CHK(hipDeviceSynchronize());
        std::vector<uint64_t> rowbuf((size_t)NJr);
        int64_t bad = 0;
        for (int64_t i : {(int64_t)0, (int64_t)517, (int64_t)1023}) {
            CHK(hipMemcpy(rowbuf.data(), d + i * NJr, (size_t)NJr * 8,
                          hipMemcpyDeviceToHost));
            for (int64_t j = 0; j < NJr; j++)
                bad += rowbuf[(size_t)j] != mix((uint64_t)(i + NIr * j) + SEED);
        }
        printf("TRUE  winner rows 0/517/1023 vs host: %s\n",
               bad ? "FAIL" : "byte-identical");
        fflush(stdout);
        if (bad) return 1;
    }

    /* ---- WPAT: the store phase alone, per store policy ------------------ */
    {
        const int64_t nti = NIr / 64, njc = NJr / 128 / 32;
        const dim3 g((uint32_t)(nti * njc)), b(64, 16);
        const int64_t n16 = rbytes / 16;
        std::vector<double> t[N_ST + 1];
        for (int r = -1; r < ROUNDS; r++) { /* round -1 warms up */
            double m[N_ST + 1];
            m[0] = time_ms([&] { hipLaunchKernelGGL((w_vs<32, 0>), g, b, 0, 0, d, NJr, nti); }, 1);
            m[1] = time_ms([&] { hipLaunchKernelGGL((w_vs<32, 1>), g, b, 0, 0, d, NJr, nti); }, 1);
            m[2] = time_ms([&] { hipLaunchKernelGGL((w_vs<32, 2>), g, b, 0, 0, d, NJr, nti); }, 1);
            m[3] = time_ms([&] { hipLaunchKernelGGL((w_vs<32, 3>), g, b, 0, 0, d, NJr, nti); }, 1);
            m[4] = time_ms([&] { hipLaunchKernelGGL(w_1d, dim3((uint32_t)(n16 / 256)), dim3(256), 0, 0, (v4u *)d, n16); }, 1);
            if (r >= 0)
                for (int v = 0; v <= N_ST; v++) t[v].push_back(m[v]);
        }
        for (int st = 0; st < N_ST; st++) {
            char nm[64];
            snprintf(nm, sizeof nm, "tile write pattern st=%s", ST_NAME[st]);
            row("WPAT", nm, "8GiB", (double)rbytes, stat_of(t[st]));
        }
        row("WPAT", "contiguous 1-D write plain", "8GiB", (double)rbytes,
            stat_of(t[N_ST]));
    }

    /* ---- SIZE: where streaming starts to pay ---------------------------- */
    {
        struct Shape { int64_t ni, nj; const char *name; };
        const Shape shapes[6] = {
            {256, 1 << 16, "128MiB"}, {256, 1 << 17, "256MiB"},
            {512, 1 << 17, "512MiB"}, {512, 1 << 18, "1GiB"},
            {512, 1 << 19, "2GiB"},   {1024, 1 << 20, "8GiB"}};
        const int var[3][3] = {{0, 0, 0},
                               {best_st, 0, 0},
                               {win_st, win_ld, win_sw}};
        const int nvar = (win_st == best_st && !win_ld && !win_sw) ? 2 : 3;
        for (const Shape &sh : shapes) {
            const int jc = depth_index(sh.ni, sh.nj);
            const double bytes = (double)sh.ni * sh.nj * 8;
            int reps = (int)((2ll << 30) / (int64_t)bytes);
            reps = reps < 1 ? 1 : reps > 16 ? 16 : reps;
            std::vector<double> t[3];
            for (int r = -1; r < ROUNDS; r++)
                for (int v = 0; v < nvar; v++) {
                    const double ms = time_ms(
                        [&] {
                            TAB[jc][var[v][0]][var[v][1]][var[v][2]](
                                s, d, sh.ni, sh.nj, sh.nj);
                        },
                        reps);
                    if (r >= 0) t[v].push_back(ms);
                }
            for (int v = 0; v < nvar; v++) {
                char nm[64];
                snprintf(nm, sizeof nm, "c%d st=%s ld=%s %s", JCS[jc],
                         ST_NAME[var[v][0]], LD_NAME[var[v][1]],
                         SW_NAME[var[v][2]]);
                row("SIZE", nm, sh.name, 2.0 * bytes, stat_of(t[v]));
            }
        }
    }

    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    CHK(hipFree(s));
    CHK(hipFree(d));
    return 0;
}
