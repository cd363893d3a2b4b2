/* pencilhip.h — C ABI of the MI355X-native global-transpose engine.
 *
 * This is the drop-in boundary replacing the engine underneath
 * PencilArrays.jl's Transpositions.transpose! hot path.  The reference has no
 * FFI of its own (pure Julia); each entry point below names the reference
 * function whose role it takes, so a Julia host can bind 1:1 via ccall
 * (see INTEGRATION.md for the ccall stubs), and any C/C++/Python host can
 * call it directly.  All lengths are int64 (the reference's MPI counts are
 * Cint and warn near 2^31, Pencils.jl:363-380; this ABI has no such cliff).
 *
 * Conventions: dims/permutations 0-based; ranges half-open; a permutation q
 * maps memory axes to logical dims (q[i] = logical dim at memory position i,
 * memory axis 0 fastest — the column-major Julia parent, arrays.jl:134-138).
 * Parent arrays are flat device buffers of length prod(local memory dims).
 *
 * Thread model: one process (or host thread) per GPU rank; a plan is
 * rank-local like the reference's Transposition (Transpositions.jl:70-92).
 * All execution is asynchronous on the caller's HIP stream.
 */

#ifndef PENCILHIP_H
#define PENCILHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pa_topology pa_topology; /* MPITopology{M}, MPITopologies.jl:72-119 */
typedef struct pa_pencil pa_pencil;     /* Pencil{N,M},    Pencils.jl:151-251    */
typedef struct pa_comm pa_comm;         /* one RCCL communicator = one 1-D
                                         * subcommunicator (MPITopologies.jl:244-251) */
typedef struct pa_plan pa_plan;         /* Transposition,  Transpositions.jl:94-119 */

typedef int pa_status; /* 0 = ok; nonzero = error, see pa_last_error() */

const char *pa_last_error(void);

/* ---- topology: process grid, rank maps ------------------------------- */
/* MPITopology(comm, pdims) with reorder=false => row-major rank order
 * (MPITopologies.jl:125-131); subgroup rank along a dim == coordinate
 * (:229-242). */
pa_status pa_topology_create(int m, const int64_t *pdims, pa_topology **out);
void pa_topology_destroy(pa_topology *t);
int pa_topology_nranks(const pa_topology *t);
pa_status pa_topology_coords(const pa_topology *t, int rank, int64_t *coords);

/* ---- pencil: decomposition metadata ---------------------------------- */
/* Pencil(topology, size_global, decomp_dims; permute) (Pencils.jl:238-251).
 * perm may be NULL (NoPermutation). */
pa_status pa_pencil_create(pa_topology *t, int n, const int64_t *size_global,
                           const int32_t *decomp_dims, const int32_t *perm,
                           pa_pencil **out);
void pa_pencil_destroy(pa_pencil *p);
/* range_local(p, rank, order) (Pencils.jl:512-514): n half-open ranges into
 * lo[n], hi[n]; memory_order != 0 permutes (axes_local_perm). */
pa_status pa_pencil_range_local(const pa_pencil *p, int rank, int memory_order,
                                int64_t *lo, int64_t *hi);
/* size_local / length_local (Pencils.jl:495,546) incl. nothing extra. */
pa_status pa_pencil_size_local(const pa_pencil *p, int rank, int memory_order,
                               int64_t *out);
int64_t pa_pencil_length_local(const pa_pencil *p, int rank);

/* ---- RCCL communicator bootstrap ------------------------------------- */
/* The host exchanges the opaque unique id out-of-band (MPI, TCP store, ...)
 * and every member of one 1-D subgroup calls pa_comm_create with the same id
 * and its subgroup rank (= its Cartesian coordinate along the transposed
 * dimension).  Replaces MPI.Cart_sub / topology.subcomms[R]
 * (MPITopologies.jl:244-251, Transpositions.jl:295-298). */
int pa_unique_id_size(void);
pa_status pa_get_unique_id(char *id /* pa_unique_id_size() bytes */);
pa_status pa_comm_create(const char *id, int nranks, int rank, pa_comm **out);
void pa_comm_destroy(pa_comm *c);

/* ---- transposition plan ---------------------------------------------- */
/* Transposition(Ao, Ai) (Transpositions.jl:94-119): validates compatibility
 * (:182-199), finds the transposed dimension R (:111), and precomputes every
 * pack/exchange/unpack block (:346-536).  elem_size in bytes (the path is
 * pure data movement; dtype enters via size only).  extra_dims (E slowest
 * axes, arrays.jl:105-106) may be NULL with e = 0.
 * Unlike the reference, which re-plans on every transpose! call (:165-167),
 * a plan is reusable and allocation-free in steady state.
 * flags bit 0 (PA_PLAN_ALIASED): src and dst parents may alias (the
 * reference's in-place / ManyPencilArray transposes, multiarrays.jl:106-143,
 * Transpositions.jl:250-264): the self block then stages through the
 * recv-buffer tail so every src read completes before any dst write.
 * Env PENCILHIP_EXCHANGE_CHUNKS=N (read at plan creation, default 1):
 * split the exchange into N chunk groups and unpack each chunk while later
 * chunks are in flight (the reference's Waitany overlap,
 * Transpositions.jl:510-517).
 * flags bit 1 (PA_PLAN_GROUP_CVT): on a plan with a wire pair
 * (pa_plan_create_wire) the converting kernels of a stage run as grouped
 * launches, see there; on any other plan the bit has no effect.
 * flags bit 2 (PA_PLAN_GROUP_SOA): on a scalar plan the split and join stage
 * calls run as grouped launches and accept a keep plan, see "split and join
 * transposes"; on any other plan the bit has no effect. */
#define PA_PLAN_ALIASED 1
#define PA_PLAN_GROUP_CVT 2
#define PA_PLAN_GROUP_SOA 4
pa_status pa_plan_create(const pa_pencil *pin, const pa_pencil *pout,
                         int64_t elem_size, int e, const int64_t *extra_dims,
                         int rank, int flags, pa_plan **out);
/* Composite elements: an element of ncomp scalars of scalar_size bytes each,
 * COMPONENTS FASTEST (array of structs) — the reference's isbits element
 * types such as SVector{3,Float64}, which it transposes as one 24-byte
 * element (test/ode.jl).  scalar_size must be 1, 2, 4, 8 or 16 when
 * ncomp > 1.  Every descriptor, offset and count of the plan stays in ELEMENT
 * units; only byte sizes (staging buffers, exchange) carry the factor
 * scalar_size * ncomp.  pa_plan_create(.., elem_size, ..) is exactly
 * pa_plan_create_comp(.., elem_size, 1, ..).
 * A host with a composite element should pass the pair — (8, 3) for
 * SVector{3,Float64} — rather than elem_size = 24: the pair reaches the
 * wide-element LDS tile (PA_KERNEL_TILE_WIDE), while a plain composite
 * elem_size keeps the byte-ify fallback. */
pa_status pa_plan_create_comp(const pa_pencil *pin, const pa_pencil *pout,
                              int64_t scalar_size, int64_t ncomp, int e,
                              const int64_t *extra_dims, int rank, int flags,
                              pa_plan **out);

/* Reduced-precision wire: the plan of ncomp scalars of a STORED type per
 * element whose staging buffers and messages carry a narrower WIRE type — a
 * field kept in float64 exchanged as float32 halves every message, the
 * standard lever of pseudo-spectral codes (the reference has no such option;
 * its transpose! moves eltype(src) as is).  Wire pairs (stored -> wire): */
#define PA_WIRE_F64_F32  1 /* float64 -> float32  */
#define PA_WIRE_F32_F16  2 /* float32 -> float16  */
#define PA_WIRE_F32_BF16 3 /* float32 -> bfloat16 */
/* What one converting copy does (pa_device_copy_wire): */
#define PA_WIRE_NARROW 0 /* stored -> wire: every pack, the aliased self pack */
#define PA_WIRE_WIDEN  1 /* wire -> stored: every unpack, aliased self unpack */
#define PA_WIRE_ROUND  2 /* stored -> stored through the wire type: the fused
                          * local copy and same-decomposition plans */
/* pa_plan_create_wire builds the tables of pa_plan_create_comp(.., stored
 * scalar size, ncomp, ..): pa_plan_copydesc[_many] return the same
 * descriptors (element units).  Only byte sizes differ: pa_plan_buffer_sizes,
 * pa_plan_buffer_sizes_many and pa_plan_peer_message report WIRE bytes, and
 * the hipMalloc fallback of pa_transpose_execute and the ncclSend/ncclRecv
 * counts use the wire element size.  ncomp = 1 is a real field, 2 a complex
 * one (complex128 with PA_WIRE_F64_F32 is complex64 on the wire), and
 * elem_dims multiply in.
 * Contract: with round_w(x) = x converted to the wire type (round to nearest
 * even, subnormals of the wire type kept, beyond its range +-inf, +-0 and
 * +-inf preserved, NaN stays NaN with sign and payload unspecified) and back,
 *     dest == T(round_w(src))   bit for bit on every non-NaN element,
 * T being the transposition of the same plan without a wire pair.  EVERY
 * element is rounded — the fused local copy, the staged self block of an
 * aliased plan, a same-decomposition plan — so the result does not depend on
 * the process grid, and since round_w is idempotent a chain x->y->z rounds
 * once.  pa_transpose_execute[_many], the three stage calls,
 * pa_transpose_wait, timing and PA_PLAN_ALIASED work on a wire plan.
 * PENCILHIP_EXCHANGE_CHUNKS does NOT apply: the exchange is a single group.
 * With PA_PLAN_GROUP_CVT in flags the PA_KERNEL_CVT_LINEAR entries of one
 * stage with the same (op, scalars per access) share ONE grouped launch, and
 * so do its PA_KERNEL_CVT_TILE entries of one op, in first-appearance order
 * (the rule the ordinary plan applies to (kind, word));
 * PA_KERNEL_CVT_GENERIC entries stay one launch each.  The selection per
 * descriptor, the tables, the byte sizes and the result are those of the plan
 * without the flag.  pa_transpose_execute then runs the n = 1 stage path
 * (pa_transpose_execute_many), so a single field is grouped too; its
 * hipMalloc fallback, sized in wire bytes, serves that path. */
pa_status pa_plan_create_wire(const pa_pencil *pin, const pa_pencil *pout,
                              int wire, int64_t ncomp, int e,
                              const int64_t *extra_dims, int rank, int flags,
                              pa_plan **out);
/* The wire pair of a plan, or 0 for an ordinary plan. */
int pa_plan_wire(const pa_plan *p);
/* 1 for a plan with a wire pair created with PA_PLAN_GROUP_CVT, else 0 (an
 * ordinary or keep plan ignores the flag). */
int pa_plan_group_cvt(const pa_plan *p);
/* 1 for a plan created with PA_PLAN_GROUP_SOA on which the flag has an
 * effect: a scalar plan (ncomp == 1) of 4-, 8- or 16-byte scalars that is not
 * aliased and has no wire pair; else 0. */
int pa_plan_group_soa(const pa_plan *p);

/* Scaled transpose: dest = alpha * T(src), the normalisation of an inverse
 * FFT folded into the pass that writes the destination anyway (the reference
 * has no such option: PencilFFTs scales in a broadcast of its own after the
 * last transpose).  Real scalar types of a scale: */
#define PA_SCALAR_F32 1 /* float32 */
#define PA_SCALAR_F64 2 /* float64 */
/* pa_plan_set_scale is valid on a plan of pa_plan_create, pa_plan_create_comp
 * or pa_plan_create_keep whose element size is a multiple of the scalar
 * size; an element is then nscal = element bytes / scalar bytes scalars
 * (a complex element two, elem_dims multiply in).
 * Contract: with S the scalar type, a = S(alpha) (alpha rounded to nearest
 * even) and T the transposition of the same plan without a scale,
 *     dest == T(src (*) a)   bit for bit on every non-NaN scalar,
 * NaN staying NaN with sign and payload unspecified; (*) is ONE IEEE
 * multiply per real scalar: round to nearest even, subnormals kept, +-0 and
 * +-inf by the IEEE rules.  A complex element is scaled component by
 * component; it is not a complex multiply.  Every element is multiplied
 * exactly once, on the DESTINATION side: the fused local copy, the aliased
 * self unpack and every unpack.  Packs and the aliased self pack stay the
 * ordinary kernels, so staging buffers and messages carry unscaled bytes,
 * identical to those of the plan without a scale (a host that runs its own
 * exchange through the stage calls sees no difference), and the result does
 * not depend on the process grid.  On a keep plan dest[i] = a * src[i] for i
 * in K; the fill is unchanged.
 * alpha == 1.0 means "no scale": the plan then runs exactly the code, tables
 * and launches it runs without this call, and pa_plan_scale returns 0.
 * alpha is a kernel argument and not part of the stage tables: a change
 * between two values != 1 keeps the cached tables, a change between scaled
 * and unscaled drops them (pa_plan_stage_table_count becomes 0).
 * A scaled plan's descriptors, byte sizes and pack launches are those of the
 * plan without a scale.  Its local and unpack copies run the scaling kernels
 * (pa_copy_kernel_kind_scale per descriptor), grouped from the start: the
 * PA_KERNEL_SCALE_LINEAR entries of one stage with the same scalars per
 * access share ONE launch, and so do its PA_KERNEL_SCALE_TILE entries, in
 * first-appearance order; PA_KERNEL_SCALE_GENERIC entries stay one launch
 * each; a keep plan's grouped PA_KERNEL_FILL launch stays as it is.
 * pa_transpose_execute runs the n = 1 stage path (pa_transpose_execute_many)
 * and PENCILHIP_EXCHANGE_CHUNKS does not apply.  pa_transpose_execute_many,
 * the three stage calls, pa_transpose_wait, timing and PA_PLAN_ALIASED work.
 * Errors: a plan with a wire pair (that would be two roundings per element
 * and another contract; left out deliberately), an unknown scalar code, an
 * element size that is no multiple of the scalar size, a NaN or infinite
 * alpha. */
pa_status pa_plan_set_scale(pa_plan *p, int scalar, double alpha);
/* 1 for a scaled plan (*scalar, *alpha written where non-NULL), else 0. */
int pa_plan_scale(const pa_plan *p, int *scalar, double *alpha);

/* Truncated transpose: move only a kept product set of indices — the other
 * standard lever of a pseudo-spectral code (after the 2/3 rule a third of the
 * modes along every transformed dimension are known zeros; the reference has
 * no such option, its transpose! moves every element of src).
 * The keep set is K = K_0 x ... x K_{N-1} over the LOGICAL dims with
 *     K_d = [0, keep_lo[d]) U [N_d - keep_hi[d], N_d),
 * keep_lo, keep_hi >= 0 and keep_lo[d] + keep_hi[d] <= N_d: keep_hi = 0 for an
 * r2c dim, low and high wavenumbers for a c2c dim, (N_d, 0) keeps everything.
 * extra_dims and element components are never truncated.
 * Contract, T being the transposition of the same pencil pair:
 *     dest[i] = src[i] bit for bit      for global index i in K,
 *     dest[i] = +0 (all zero bytes)     for i not in K with PA_FILL_ZERO,
 *     dest[i] unchanged                 for i not in K with PA_FILL_NONE.
 * Every block of the ordinary plan (a peer's send region, a peer's recv
 * region, the self block) is intersected with K: up to 2^N sub-boxes, low
 * range before high range, dim 0 varying fastest, empty ones dropped; the two
 * ranges of a dim merge when keep_lo + keep_hi == N_d.  Each sub-box is a
 * staging block of its own (offset o_s, count c_s; the sub-boxes of a peer
 * are consecutive, peers in ascending order) with one ordinary descriptor:
 * field f of n sits at n*o_s + f*c_s, and peer k's message is still ONE
 * contiguous range of the KEPT bytes (pa_plan_peer_message); a peer with
 * nothing kept has a zero-byte message and is left out of the exchange on
 * both sides.  Sender and receiver derive the same sub-boxes.
 * pa_plan_buffer_sizes[_many], pa_plan_peer_message, the three stage calls,
 * pa_transpose_execute[_many], pa_transpose_wait, timing, PA_PLAN_ALIASED and
 * pa_plan_stage_launches work with the kept sizes; pa_transpose_execute runs
 * the n = 1 stage path and its hipMalloc fallback is sized in kept bytes.
 * With PA_FILL_ZERO the local stage also zero-fills the windows of the
 * destination outside K (pa_plan_filldesc) with ONE grouped launch
 * (PA_KERNEL_FILL); fill and copy windows are disjoint, so no ordering
 * between them is needed.  PENCILHIP_EXCHANGE_CHUNKS does not apply.  There
 * is no keep plan with a wire pair yet.  With the full keep set the tables,
 * sizes and launches equal those of pa_plan_create_comp. */
#define PA_FILL_NONE 0
#define PA_FILL_ZERO 1
pa_status pa_plan_create_keep(const pa_pencil *pin, const pa_pencil *pout,
                              int64_t scalar_size, int64_t ncomp, int e,
                              const int64_t *extra_dims, int rank, int flags,
                              const int64_t *keep_lo, const int64_t *keep_hi,
                              int fill, pa_plan **out);
/* 1 for a keep plan (lo[N], hi[N], *fill written where non-NULL), else 0. */
int pa_plan_keep(const pa_plan *p, int64_t *lo, int64_t *hi, int *fill);
void pa_plan_destroy(pa_plan *p);

/* Subgroup communicator for the exchange (required when the subgroup size
 * P > 1; its nranks must equal P and its rank my coordinate along R). */
pa_status pa_plan_set_comm(pa_plan *p, pa_comm *c);

/* Staging buffers (the send_buf/recv_buf of Pencils.jl:187-189).  Either ask
 * the sizes and provide device memory, or skip: execute() allocates with
 * hipMalloc on first use. */
pa_status pa_plan_buffer_sizes(const pa_plan *p, int64_t *send_bytes,
                               int64_t *recv_bytes);
pa_status pa_plan_set_buffers(pa_plan *p, void *send_buf, void *recv_buf);

/* transpose!(t) (Transpositions.jl:161-180): pack -> RCCL grouped
 * send/recv -> fused local copy -> unpack, asynchronous on `stream`
 * (hipStream_t; pass 0 for the default stream; from PyTorch use
 * torch.cuda.current_stream().cuda_stream).  src/dst are device pointers to
 * the parent flats; they must not alias. */
pa_status pa_transpose_execute(pa_plan *p, const void *src_parent,
                               void *dst_parent, void *stream);
/* MPI.Waitall(t) (Transpositions.jl:128-131): wait for completion. */
pa_status pa_transpose_wait(pa_plan *p, void *stream);

/* ---- per-stage timing -------------------------------------------------- */
/* The TimerOutputs.@timeit_debug analogue (Transpositions.jl:173-177,327,
 * 337): opt-in HIP-event timing of the last execute's stages.  Call
 * pa_plan_stage_times after pa_transpose_wait; out = {pack_ms, local_ms,
 * exchange_ms, unpack_ms} (-1 for stages the plan does not run; exchange is
 * timed on the engine's comm stream, overlapping local_ms by design). */
pa_status pa_plan_enable_timing(pa_plan *p, int enable);
pa_status pa_plan_stage_times(pa_plan *p, double out[4]);

/* ---- plan introspection (host-side, for parity tests) ---------------- */
int pa_plan_nproc_sub(const pa_plan *p);      /* P (1 => purely local)  */
int pa_plan_r_dim(const pa_plan *p);          /* R, or -1 if same decomp */
int pa_plan_my_k(const pa_plan *p);
pa_status pa_plan_block_info(const pa_plan *p, int k, int64_t out[8]);
/* which: 0 = local fused copy, 1 = pack of peer k, 2 = unpack of peer k,
 * 3 = staged self pack (aliased mode), 4 = staged self unpack.
 * Returns the normalized strided-copy descriptor (element units):
 * nd, dims[nd], sstrides[nd], soffset, dstrides[nd], doffset. */
pa_status pa_plan_copydesc(const pa_plan *p, int which, int k, int64_t *nd,
                           int64_t *dims, int64_t *sstr, int64_t *soff,
                           int64_t *dstr, int64_t *doff);

/* ---- multi-field transposes -------------------------------------------- */
/* n separately allocated fields of ONE pencil pair in one call — what a host
 * does today with n transpose! calls (Transpositions.jl:161-180; the
 * reference batches only fields allocated together, extra_dims,
 * arrays.jl:105-106).  One plan (element units, unchanged) serves any n:
 *
 *  - staging is n times the plan's sizes.  A staging block that starts at
 *    element offset o with c elements in the single-field plan (a peer's
 *    send block, a peer's recv block, the aliased self block in the recv
 *    tail) holds field f at n*o + f*c; n = 1 is today's layout;
 *  - peer k's message is the contiguous range [n*o_k, n*(o_k+c_k)): ONE send
 *    and ONE recv per peer whatever n is (Transpositions.jl:419-428 posts
 *    one per peer per field);
 *  - each stage is one grouped kernel launch per kernel signature (kind,
 *    word size) over a device-resident table of descriptors.  Selection per
 *    descriptor is that of pa_copy_kernel_kind_comp.  COPY_1D/LINEAR, TILE
 *    and TILE_VS at sweep depth 1 are grouped; any other selection runs as
 *    an ordinary launch from the same stage call.
 *
 * Staging MUST come from pa_plan_set_buffers with at least
 * pa_plan_buffer_sizes_many bytes (the hipMalloc fallback of
 * pa_transpose_execute sizes for one field and is refused here).  Tables are
 * cached per plan, keyed on n, the stage and every pointer involved; steady-
 * state calls on the same arrays allocate nothing.  pa_plan_set_buffers
 * drops the cache (and waits for the device). */

/* send_buf/recv_buf sizes for n fields (Pencils.jl:187-189, times n). */
pa_status pa_plan_buffer_sizes_many(const pa_plan *p, int n,
                                    int64_t *send_bytes, int64_t *recv_bytes);
/* The message exchanged with subgroup peer k for n fields, in BYTES into the
 * staging buffers: out = {send_off, send_bytes, recv_off, recv_bytes} — the
 * buffer ranges of MPI.Isend / MPI.Irecv! in Transpositions.jl:463-479.  All
 * zero for k == my coordinate (the self block is never a message).  A host
 * with its own transport (GPU-aware MPI) needs only this and the stages. */
pa_status pa_plan_peer_message(const pa_plan *p, int n, int k, int64_t out[4]);

/* The stages of transpose! separately, asynchronous on `stream`:
 *   pack_many   = step 1 of pa_transpose_execute: every pack of every field
 *                 into send_buf (transpose_send!, Transpositions.jl:346-431),
 *                 and in aliased mode the staged self packs (:394-404);
 *   local_many  = step 3: the fused local copies, or in aliased mode the
 *                 staged self unpacks;
 *   unpack_many = step 4: every unpack of every field from recv_buf
 *                 (transpose_recv!, :489-536).
 * ORDERING A FOREIGN EXCHANGE IS THE HOST'S JOB: the sends may start only
 * once pack_many has completed on `stream` (synchronize it, or make the
 * transport's stream wait on an event), and unpack_many may be enqueued only
 * after every recv has landed in recv_buf.  local_many touches no remote
 * block and may overlap the exchange.  In aliased mode enqueue pack_many
 * before local_many and unpack_many: they write the destinations. */
pa_status pa_transpose_pack_many(pa_plan *p, int n, const void *const *srcs,
                                 void *stream);
pa_status pa_transpose_local_many(pa_plan *p, int n, const void *const *srcs,
                                  void *const *dsts, void *stream);
pa_status pa_transpose_unpack_many(pa_plan *p, int n, void *const *dsts,
                                   void *stream);

/* transpose!(t) for n fields: pack_many -> ONE grouped RCCL exchange (one
 * ncclSend/ncclRecv per peer at the pa_plan_peer_message ranges, on the
 * engine's comm stream, event-ordered as in pa_transpose_execute) ->
 * local_many -> unpack_many.  pa_transpose_wait and pa_plan_stage_times work
 * after it unchanged.  PENCILHIP_EXCHANGE_CHUNKS does NOT apply: the
 * exchange is always a single group.  PA_PLAN_ALIASED plans are supported
 * (srcs and dsts may then alias in any combination): every pack and self
 * pack of every field is enqueued before any write of a destination. */
pa_status pa_transpose_execute_many(pa_plan *p, int n,
                                    const void *const *srcs,
                                    void *const *dsts, void *stream);

/* Introspection (host-only, no GPU).  pa_plan_copydesc_many: the descriptor
 * of field f of n, in the form and with the `which` of pa_plan_copydesc
 * (0..4): the single-field descriptor with its staging-side offset moved by
 * (n-1)*o + f*c. */
pa_status pa_plan_copydesc_many(const pa_plan *p, int n, int f, int which,
                                int k, int64_t *nd, int64_t *dims,
                                int64_t *sstr, int64_t *soff, int64_t *dstr,
                                int64_t *doff);
/* The launches a stage makes for these arrays (stage: 0 = pack, 1 = local,
 * 2 = unpack), one row each: {kind, grouped 0/1, entries, workgroups}.  A
 * grouped row of the linear family reports PA_KERNEL_LINEAR.  Pointers are
 * used for alignment only and never dereferenced, like pa_copy_kernel_kind;
 * srcs, dsts or single pointers may be NULL (taken as 256-byte aligned).
 * Staging is taken from pa_plan_set_buffers, else assumed 256-byte aligned.
 * At most max_rows rows are written; *nrows is the full count.  The stage
 * calls execute exactly this list.  A wire plan reports its converting
 * kernels (PA_KERNEL_CVT_*) as ungrouped rows, one per descriptor; created
 * with PA_PLAN_GROUP_CVT it reports {PA_KERNEL_CVT_LINEAR or
 * PA_KERNEL_CVT_TILE, 1, entries, workgroups} per signature, workgroups being
 * the sum of the entries' grids, and PA_KERNEL_CVT_GENERIC rows as before.  A keep
 * plan has one entry per sub-box and field, and its local stage ends with
 * ONE grouped PA_KERNEL_FILL row holding the fill entries of every field. */
#define PA_STAGE_PACK   0
#define PA_STAGE_LOCAL  1
#define PA_STAGE_UNPACK 2
pa_status pa_plan_stage_launches(const pa_plan *p, int n, int stage,
                                 const void *const *srcs, void *const *dsts,
                                 int max_rows, int64_t (*rows)[4], int *nrows);

/* Keep plans (pa_plan_create_keep): pa_plan_copydesc[_many] fail on them and
 * name pa_plan_copydesc_sub.  pa_plan_nsub: the non-empty sub-boxes behind
 * `which` (0..4 as in pa_plan_copydesc; peer k for 1 and 2); 0 on any other
 * plan.  pa_plan_copydesc_sub: sub-box s of field f of n, in the form of
 * pa_plan_copydesc_many.  pa_plan_nfill / pa_plan_filldesc: the zero-filled
 * windows of the output parent, destination-only descriptors in element
 * units (unit axes dropped, contiguous axes merged): for d = 0..N-1, (kept in
 * dims < d) x (dropped range of dim d) x (everything in dims > d), clipped to
 * this rank, empty ones dropped; none with PA_FILL_NONE. */
int pa_plan_nsub(const pa_plan *p, int which, int k);
pa_status pa_plan_copydesc_sub(const pa_plan *p, int n, int f, int which,
                               int k, int s, int64_t *nd, int64_t *dims,
                               int64_t *sstr, int64_t *soff, int64_t *dstr,
                               int64_t *doff);
int pa_plan_nfill(const pa_plan *p);
pa_status pa_plan_filldesc(const pa_plan *p, int i, int64_t *nd,
                           int64_t *dims, int64_t *dstr, int64_t *doff);

/* Stage tables this plan holds in its cache (at most 12, least recently used
 * evicted): one per (n, stage, array set) that has run.  A repeated call on
 * the same arrays leaves it unchanged — nothing was built or allocated. */
int pa_plan_stage_table_count(const pa_plan *p);

/* Stage tables this plan has built since it was created, evicted and dropped
 * ones included.  At the cache's capacity a build replaces a table and leaves
 * pa_plan_stage_table_count() unchanged; this counter still moves, so a call
 * that leaves it unchanged was served from the cache. */
int64_t pa_plan_stage_table_builds(const pa_plan *p);

/* ---- split and join transposes ---------------------------------------- */
/* A vector field lives in two forms: an array of structs A, n scalars of S
 * bytes per element with the components fastest (the reference's
 * PencilArray{SVector{n,S}}, here pa_plan_create_comp), and n separately
 * allocated scalar arrays F_0 .. F_{n-1} (pa_transpose_execute_many).  A split
 * transpose reads A on the input pencil and writes the F_c on the output
 * pencil, a join transpose the reverse; with T the ordinary transposition and
 * A[c] component c of A,
 *     split:  F_c == T(A[c])      join:  A[c] == T(F_c)     bit for bit,
 * whatever the process grid.  The reference has neither: a host interleaves
 * or de-interleaves in a pass of its own.
 *
 * Both run on an ORDINARY SCALAR plan, pa_plan_create(.., S, ..) with S = 4, 8
 * or 16, and n >= 2 is an argument of the call.  Staging buffers and messages
 * are byte for byte those of the n-field plan applied to the component copies
 * A[c]: pa_plan_buffer_sizes_many(p, n) and pa_plan_peer_message(p, n, k) hold
 * unchanged, and staging MUST come from pa_plan_set_buffers.  So a split's
 * unpack is pa_transpose_unpack_many, a join's pack is pa_transpose_pack_many,
 * and either may face an ordinary n-field peer.  The layout change sits in
 *   pack_split   every pack: A -> the n component slots of each send block;
 *   local_split  the fused local copy A -> F_c;
 *   local_join   the fused local copy F_c -> A;
 *   unpack_join  every unpack: the n slots of each recv block -> A,
 * one launch per block carrying all n components (pa_copy_kernel_kind_soa
 * tells which kernel).  Ordering a foreign exchange is the host's job exactly
 * as for the _many stages.  execute_split / execute_join run pack, the
 * single-group exchange of pa_transpose_execute_many, local, unpack;
 * pa_transpose_wait and pa_plan_stage_times work after them.
 * Refused with an error: a PA_PLAN_ALIASED plan (the two sides have different
 * element sizes and cannot alias), a keep plan (unless the plan was created
 * with PA_PLAN_GROUP_SOA, below), a wire plan, a plan with a scale set, a composite plan (ncomp > 1), n < 2, S not 4, 8 or 16.
 *
 * A scale is given PER CALL, to the *_scaled forms below, exactly as n is: the
 * plan stays the ordinary scalar plan, because a plan on which
 * pa_plan_set_scale was called is refused by every split / join call, plain
 * or scaled (its scale names the stages of an ordinary transpose, which are
 * not the ones a split multiplies in).  R = scalar is PA_SCALAR_F32 or
 * PA_SCALAR_F64 and S must be one or two R: (S, R) = (4, F32), (8, F32)
 * (complex64), (8, F64) or (16, F64) (complex128).  With a = R(alpha) rounded
 * to nearest even and (*) ONE IEEE multiply per real scalar (round to nearest
 * even, subnormals kept, a complex scalar component by component), the
 * contract of pa_plan_set_scale:
 *     split:  F_c == T(A[c] (*) a)      join:  A[c] == T(F_c (*) a)
 * bit for bit on every non-NaN scalar (a NaN stays NaN, sign and payload
 * unspecified), whatever the process grid; every scalar is multiplied exactly
 * once, in the two stages that carry the layout change:
 *   join   local_join and unpack_join multiply, the destination side as in a
 *          scaled plan.  The pack is pa_transpose_pack_many: staging and
 *          messages carry UNSCALED bytes, identical to the plain join's.
 *   split  pack_split and local_split multiply, the SOURCE side, because the
 *          split's unpack is the ordinary pa_transpose_unpack_many of an
 *          ordinary plan and cannot multiply.  Staging and messages therefore
 *          carry SCALED bytes: those of the n-field plan applied to the scaled
 *          component copies A[c] (*) a, and a peer that unpacks with the
 *          ordinary n-field stage receives the scaled fields.
 * alpha == 1.0 means "no scale": the call runs exactly the code of the plain
 * call, NaN payloads included.  alpha is a kernel argument: calls with
 * different alpha on one plan build and allocate nothing.  The kernel
 * selection is that of the plain calls, unchanged (pa_copy_kernel_kind_soa
 * reports kind, V and tile shape for both); the scaled call launches the
 * scaling form of the selected kernel.
 * Errors, raised before any pointer is touched: everything the plain calls
 * refuse, with their messages; then an unknown scalar code, a NaN or infinite
 * alpha, an (S, R) pair outside the four above.
 *
 * PA_PLAN_GROUP_SOA (opt-in; pa_plan_group_soa(p) == 1) changes two things
 * about the ten calls below, and nothing about any other call, table,
 * descriptor or byte size of the plan:
 *  - the four stages run through stage tables in the plan's cache, keyed on
 *    (n, direction, stage, A, the field pointers) and dropped by
 *    pa_plan_set_buffers like the others.  The PA_KERNEL_SOA_LINEAR entries of
 *    one stage with the same V share ONE grouped launch and so do all its
 *    PA_KERNEL_SOA_TILE entries, in first-appearance order;
 *    PA_KERNEL_SOA_GENERIC entries stay one launch each.  The kernels run the
 *    bodies of the ungrouped ones, so the bytes are the same.  alpha is a
 *    kernel argument and not part of a table: a repeated call, a call with
 *    another alpha, and a plain call after a scaled one on the same arrays
 *    build and allocate nothing (pa_plan_stage_table_builds);
 *  - a keep plan (pa_plan_create_keep) is accepted.  With K its keep set,
 *        split:  F_c[i] == A[c][i]    join:  A[c][i] == F_c[i]    i in K,
 *    bit for bit; the destination at i outside K reads +0 with PA_FILL_ZERO
 *    and is untouched with PA_FILL_NONE.  A scaled call multiplies the kept
 *    scalars exactly once, in the stages that multiply without a keep set;
 *    outside K the result is +0 whatever the sign of alpha.  Staging and
 *    messages are byte for byte those of the n-field keep plan on the
 *    (scaled, for a split) component copies, in kept elements, and nothing
 *    beyond them is written; either side may face an ordinary n-field keep
 *    peer.  The zero fill is ONE grouped PA_KERNEL_FILL launch at the end of
 *    local_split / local_join over the pa_plan_filldesc windows: of all n
 *    destinations for a split, and of A in elements of n * S bytes for a
 *    join.  With the full keep set everything equals the flagged ordinary
 *    plan's and there is no fill.
 * An aliased, wire, composite or 2-byte plan ignores the flag and a plan with
 * a scale set stays refused, all with the messages above. */
pa_status pa_transpose_pack_split(pa_plan *p, int n, const void *src_aos,
                                  void *stream);
pa_status pa_transpose_local_split(pa_plan *p, int n, const void *src_aos,
                                   void *const *dsts, void *stream);
pa_status pa_transpose_local_join(pa_plan *p, int n, const void *const *srcs,
                                  void *dst_aos, void *stream);
pa_status pa_transpose_unpack_join(pa_plan *p, int n, void *dst_aos,
                                   void *stream);
pa_status pa_transpose_execute_split(pa_plan *p, int n, const void *src_aos,
                                     void *const *dsts, void *stream);
pa_status pa_transpose_execute_join(pa_plan *p, int n,
                                    const void *const *srcs, void *dst_aos,
                                    void *stream);
pa_status pa_transpose_pack_split_scaled(pa_plan *p, int n, int scalar,
                                         double alpha, const void *src_aos,
                                         void *stream);
pa_status pa_transpose_local_split_scaled(pa_plan *p, int n, int scalar,
                                          double alpha, const void *src_aos,
                                          void *const *dsts, void *stream);
pa_status pa_transpose_local_join_scaled(pa_plan *p, int n, int scalar,
                                         double alpha,
                                         const void *const *srcs,
                                         void *dst_aos, void *stream);
pa_status pa_transpose_unpack_join_scaled(pa_plan *p, int n, int scalar,
                                          double alpha, void *dst_aos,
                                          void *stream);
pa_status pa_transpose_execute_split_scaled(pa_plan *p, int n, int scalar,
                                            double alpha,
                                            const void *src_aos,
                                            void *const *dsts, void *stream);
pa_status pa_transpose_execute_join_scaled(pa_plan *p, int n, int scalar,
                                           double alpha,
                                           const void *const *srcs,
                                           void *dst_aos, void *stream);

/* The launches a split / join stage makes (host-only), rows as in
 * pa_plan_stage_launches: {kind, grouped, entries, workgroups}.  Valid for
 * (PA_SOA_SPLIT, PA_STAGE_PACK), (PA_SOA_SPLIT, PA_STAGE_LOCAL),
 * (PA_SOA_JOIN, PA_STAGE_LOCAL) and (PA_SOA_JOIN, PA_STAGE_UNPACK); a split's
 * unpack and a join's pack are ordinary n-field stages and an error here that
 * names pa_plan_stage_launches.  aos and fields (fields is used by the local
 * stage only) matter for their alignment; NULL ones are taken as aligned, and
 * so is staging not yet set.  A plan without PA_PLAN_GROUP_SOA reports one
 * ungrouped row per non-empty descriptor, which is what its stage calls
 * launch (a PA_KERNEL_SOA_GENERIC row of n > 8 fields is several launches of
 * up to 8; its workgroups are those of all n).  A plan with the flag reports
 * the grouped rows, workgroups being the sum of the entries' grids, and on a
 * keep plan with PA_FILL_ZERO the PA_KERNEL_FILL row that ends the local
 * stage: n * pa_plan_nfill entries for a split, pa_plan_nfill for a join.
 * The stage calls execute exactly this list.  Errors: what the stage calls
 * refuse about the plan and n, an unknown dir or stage. */
pa_status pa_plan_stage_launches_soa(const pa_plan *p, int n, int dir,
                                     int stage, const void *aos,
                                     const void *const *fields, int max_rows,
                                     int64_t (*rows)[4], int *nrows);

/* ---- reductions (src/reductions.jl:9-38) ----------------------------- */
/* One ncclAllReduce over a communicator (normally the FULL topology comm):
 * the collective behind the reference's mapreduce/any/all.
 * dtype: 0=f64, 1=f32, 2=i64, 3=i32, 4=u8; op: 0=sum, 1=prod, 2=min, 3=max.
 * In-place allowed (send == recv). */
pa_status pa_allreduce(pa_comm *c, const void *sendbuf, void *recvbuf,
                       int64_t count, int dtype, int op, void *stream);

/* ---- standalone device copy (used by tests/benchmarks) --------------- */
/* Execute one strided-copy descriptor on device (same kernels the plan
 * uses).  All strides/offsets/dims in elements of elem_size bytes.
 *
 * Alignment: src and dst must be aligned to min(elem_size, 16) rounded down
 * to a power of two (an f64 buffer to 8 bytes, a 12-byte element to 4).
 * Wider words (16-byte linear copies, the 16-byte vector stores of the
 * 8-byte tile, the 8-byte accesses of the 1-/2-byte packed tile) are used
 * only where both base pointers, the offsets and the strides allow them, so
 * a buffer that starts one element into an allocation is fine.
 * Precondition, not checked: a 16-byte element needs 16-byte-aligned
 * pointers; its transpose tile moves 16-byte words and has no narrower
 * fallback. */
pa_status pa_device_copy(int nd, const int64_t *dims, const int64_t *sstr,
                         int64_t soff, const int64_t *dstr, int64_t doff,
                         int64_t elem_size, const void *src, void *dst,
                         void *stream);
/* The same for composite elements (see pa_plan_create_comp): strides,
 * offsets and dims in elements of scalar_size * ncomp bytes.
 * pa_device_copy is the ncomp = 1 case. */
pa_status pa_device_copy_comp(int nd, const int64_t *dims,
                              const int64_t *sstr, int64_t soff,
                              const int64_t *dstr, int64_t doff,
                              int64_t scalar_size, int64_t ncomp,
                              const void *src, void *dst, void *stream);

/* Which kernel pa_device_copy / a plan would launch for this descriptor
 * (host-only, needs no GPU; the launcher executes exactly this decision).
 * src/dst are used for their alignment only and never dereferenced.
 * out = {kind, word_bytes, byteified (0/1), sweep_depth}: word_bytes is the
 * width of the word the kernel moves per element of its (possibly
 * word-scaled) descriptor; byteified = the descriptor went through the
 * byte-ify fallback (element sizes that are no power of two <= 16);
 * sweep_depth = tiles swept per workgroup (1 for non-tile kernels). */
#define PA_KERNEL_NONE      0   /* empty descriptor */
#define PA_KERNEL_COPY_1D   1
#define PA_KERNEL_COPY_1D_NT 2
#define PA_KERNEL_LINEAR    3
#define PA_KERNEL_TILE      4   /* scalar LDS tile */
#define PA_KERNEL_TILE_VS   5   /* 8-byte vector-store tile */
#define PA_KERNEL_TILE_PK   6   /* packed 1-/2-byte tile */
#define PA_KERNEL_GENERIC   7
#define PA_KERNEL_TILE_WIDE 8   /* wide-element tile: m words per element */
pa_status pa_copy_kernel_kind(int nd, const int64_t *dims, const int64_t *sstr,
                              int64_t soff, const int64_t *dstr, int64_t doff,
                              int64_t elem_size, const void *src,
                              const void *dst, int64_t out[4]);
/* Composite-element form; pa_copy_kernel_kind is its ncomp = 1 case and the
 * first four fields mean the same.  out = {kind, word_bytes, byteified,
 * sweep_depth, words_per_element}.  With B = scalar_size * ncomp, ncomp > 1:
 *  - B in {1,2,4,8,16}: the decision of elem_size = B;
 *  - linear at element level: COPY_1D / COPY_1D_NT / LINEAR in the widest
 *    word dividing the run bytes, every byte stride/offset and both bases;
 *  - transposable and B <= 64: PA_KERNEL_TILE_WIDE with word_bytes W = the
 *    largest power of two <= 16 dividing B and both base addresses, and
 *    words_per_element m = B / W;
 *  - otherwise: LINEAR over the descriptor expanded to W-byte words (an
 *    inner axis of m words), byteified = 0.
 * words_per_element is 1 wherever the kernel does not split elements. */
pa_status pa_copy_kernel_kind_comp(int nd, const int64_t *dims,
                                   const int64_t *sstr, int64_t soff,
                                   const int64_t *dstr, int64_t doff,
                                   int64_t scalar_size, int64_t ncomp,
                                   const void *src, const void *dst,
                                   int64_t out[5]);

/* Cache policy of the kernel pa_device_copy, or an ungrouped plan entry,
 * launches for this descriptor (host-only, arguments of pa_copy_kernel_kind).
 * *out = 1: the streaming form of PA_KERNEL_TILE_VS, nontemporal loads and
 * nontemporal 16-byte vector stores (the two are one policy: the probe behind
 * it, profiles/stream_tile_probe.txt, shows neither paying alone); chosen
 * when the descriptor moves at least the stream threshold in bytes, one
 * direction.  *out = 0: plain accesses, always so for every other kind.  The
 * kind, word, byteified flag and sweep depth of pa_copy_kernel_kind do not
 * depend on it, and the bytes written are the same either way.  Grouped
 * launches of a multi-field stage (pa_transpose_*_many, entries of sweep
 * depth 1) keep plain accesses. */
pa_status pa_copy_kernel_stream(int nd, const int64_t *dims,
                                const int64_t *sstr, int64_t soff,
                                const int64_t *dstr, int64_t doff,
                                int64_t elem_size, const void *src,
                                const void *dst, int64_t *out);
/* Set the stream threshold in payload bytes and return the previous one
 * (default 512 MiB).  0 = stream wherever the vector-store tile runs,
 * negative = never.  A tuning and testing hook: process-wide, read when a
 * kernel is selected, so stage tables a plan has already built keep the
 * policy they were built with. */
int64_t pa_set_stream_min_bytes(int64_t min_bytes);

/* ---- converting copies (reduced-precision wire) ------------------------ */
/* One strided-copy descriptor with conversion (the kernels a wire plan
 * uses).  Strides, offsets and dims in ELEMENTS of ncomp scalars, components
 * fastest; src holds the stored type for NARROW and ROUND and the wire type
 * for WIDEN, dst the wire type for NARROW and the stored type otherwise.
 * Both pointers must be aligned to their scalar; wider accesses are used only
 * where the pointers, offsets and strides allow them. */
pa_status pa_device_copy_wire(int nd, const int64_t *dims,
                              const int64_t *sstr, int64_t soff,
                              const int64_t *dstr, int64_t doff, int wire,
                              int op, int64_t ncomp, const void *src,
                              void *dst, void *stream);
/* Which converting kernel runs for this descriptor (host-only; pointers are
 * used for their alignment only).  out = {kind, V, tile_i, tile_j,
 * sweep_depth}:
 *  - axis 0 contiguous on both sides (1-D included): PA_KERNEL_CVT_LINEAR, a
 *    lane moving V consecutive scalars per access.  V starts at
 *    16 / max(src scalar bytes, dst scalar bytes) and is halved down to 1
 *    until it divides the scalar run dims[0]*ncomp and the base pointer, the
 *    offset and every non-unit stride of BOTH sides, in scalars;
 *  - src contiguous along axis 0, dst along an axis ta >= 1, ncomp <= 4:
 *    PA_KERNEL_CVT_TILE, an LDS transpose of tile_i (axis 0) x tile_j (ta)
 *    elements holding f32 in LDS;
 *  - otherwise PA_KERNEL_CVT_GENERIC, elementwise: correct and slow.
 * V = 1 and tile = 0 where they do not apply; sweep_depth is 1. */
#define PA_KERNEL_CVT_LINEAR  9
#define PA_KERNEL_CVT_TILE    10
#define PA_KERNEL_CVT_GENERIC 11
pa_status pa_copy_kernel_kind_wire(int nd, const int64_t *dims,
                                   const int64_t *sstr, int64_t soff,
                                   const int64_t *dstr, int64_t doff,
                                   int wire, int op, int64_t ncomp,
                                   const void *src, const void *dst,
                                   int64_t out[5]);

/* ---- scaling copies (scaled transposes) -------------------------------- */
/* One strided-copy descriptor with a multiply (the kernels a scaled plan
 * uses): dst = src * S(alpha) per real scalar.  Strides, offsets and dims in
 * ELEMENTS of nscal scalars of type `scalar` (PA_SCALAR_*), scalars of an
 * element fastest.  Both pointers must be aligned to the scalar; wider
 * accesses are used only where the pointers, offsets and strides allow them.
 * alpha must be finite; alpha == 1.0 still runs the scaling kernel. */
pa_status pa_device_copy_scale(int nd, const int64_t *dims,
                               const int64_t *sstr, int64_t soff,
                               const int64_t *dstr, int64_t doff, int scalar,
                               int64_t nscal, double alpha, const void *src,
                               void *dst, void *stream);
/* Which scaling kernel runs for this descriptor (host-only; pointers are
 * used for their alignment only).  out = {kind, V, tile_i, tile_j,
 * sweep_depth}, the rules of pa_copy_kernel_kind_wire:
 *  - axis 0 contiguous on both sides (1-D included): PA_KERNEL_SCALE_LINEAR,
 *    a lane moving V consecutive scalars per access.  V starts at
 *    16 / scalar bytes and is halved down to 1 until it divides the scalar
 *    run dims[0]*nscal and the base pointer, the offset and every non-unit
 *    stride of BOTH sides, in scalars;
 *  - src contiguous along axis 0, dst along an axis ta >= 1, nscal <= 4:
 *    PA_KERNEL_SCALE_TILE, an LDS transpose of tile_i (axis 0) x tile_j (ta)
 *    elements holding the scalar type in LDS (rows of 512 bytes: tile_i =
 *    128 / nscal for f32 and 64 / nscal for f64, tile_j = 64);
 *  - otherwise PA_KERNEL_SCALE_GENERIC, elementwise: correct and slow;
 *  - an empty descriptor: PA_KERNEL_NONE.
 * V = 1 and tile = 0 where they do not apply; sweep_depth is 1. */
#define PA_KERNEL_SCALE_LINEAR  13
#define PA_KERNEL_SCALE_TILE    14
#define PA_KERNEL_SCALE_GENERIC 15
pa_status pa_copy_kernel_kind_scale(int nd, const int64_t *dims,
                                    const int64_t *sstr, int64_t soff,
                                    const int64_t *dstr, int64_t doff,
                                    int scalar, int64_t nscal,
                                    const void *src, const void *dst,
                                    int64_t out[5]);

/* ---- split / join copies (split and join transposes) ------------------- */
/* One strided-copy descriptor between an array of structs and n scalar
 * fields (the kernels the split and join stages use).  The descriptor is the
 * ordinary one of ONE component, in scalars of scalar_size bytes (4, 8 or
 * 16).  The array of structs holds scalar c of element e at n*e + c.
 * PA_SOA_SPLIT: the source side addresses `aos`, the destination side every
 * fields[c], and fields[c][dst index] = aos[n * (src index) + c].
 * PA_SOA_JOIN: the source side addresses every fields[c], the destination
 * side `aos`, and aos[n * (dst index) + c] = fields[c][src index].
 * All n + 1 pointers must be aligned to the scalar (16 bytes for a 16-byte
 * one, which moves as one word), else the call fails; wider accesses are used
 * only where the pointers, offsets and strides allow them. */
#define PA_SOA_SPLIT 0
#define PA_SOA_JOIN  1
pa_status pa_device_copy_soa(int nd, const int64_t *dims, const int64_t *sstr,
                             int64_t soff, const int64_t *dstr, int64_t doff,
                             int64_t scalar_size, int n, int dir, void *aos,
                             void *const *fields, void *stream);
/* The same copy with every real scalar multiplied once by a = R(alpha), in
 * registers between the load and the store (the kernel body a *_scaled split
 * or join stage runs): fields[c][..] = aos[..] (*) a, or the reverse.
 * scalar = R is PA_SCALAR_F32 or PA_SCALAR_F64 and scalar_size one or two R.
 * The kernel, V and tile shape are those pa_copy_kernel_kind_soa reports for
 * the plain copy: there is no selection of its own.  Always runs the scaling
 * kernel, alpha == 1.0 included, as pa_device_copy_scale does.  Errors beyond
 * pa_device_copy_soa's: an unknown scalar code, a NaN or infinite alpha, a
 * scalar_size that is neither one nor two R. */
pa_status pa_device_copy_soa_scale(int nd, const int64_t *dims,
                                   const int64_t *sstr, int64_t soff,
                                   const int64_t *dstr, int64_t doff,
                                   int64_t scalar_size, int n, int dir,
                                   int scalar, double alpha, void *aos,
                                   void *const *fields, void *stream);
/* Which split / join kernel runs for this descriptor (host-only; the n + 1
 * pointers are used for their alignment only, and fields may be NULL, taken
 * as aligned).  out = {kind, V, tile_i, tile_j, sweep_depth}:
 *  - n <= 4, n * scalar_size <= 64 and axis 0 contiguous on both sides (1-D
 *    included): PA_KERNEL_SOA_LINEAR, a lane moving V consecutive elements: n
 *    accesses of V scalars on the array-of-structs side and one per field.  V
 *    starts at 16 / scalar_size and is halved down to 1 until it divides the
 *    run dims[0], both offsets, every non-unit stride of both sides, and in
 *    scalars the aos pointer and every field pointer;
 *  - n <= 4, n * scalar_size <= 64, the source side contiguous along axis 0
 *    and the destination side along an axis ta >= 1: PA_KERNEL_SOA_TILE, an
 *    LDS transpose of tile_i (axis 0) x tile_j (ta) elements of n components,
 *    the shape of PA_KERNEL_TILE_WIDE for elements of n * scalar_size bytes;
 *  - otherwise PA_KERNEL_SOA_GENERIC, one lane per scalar: correct and slow;
 *  - an empty descriptor: PA_KERNEL_NONE.
 * V = 1 and tile = 0 where they do not apply; sweep_depth is 1.
 * Errors: n < 2, scalar_size not 4, 8 or 16, an unknown dir, out == NULL, a
 * pointer of a non-empty descriptor that is not aligned to the scalar. */
#define PA_KERNEL_SOA_LINEAR  16
#define PA_KERNEL_SOA_TILE    17
#define PA_KERNEL_SOA_GENERIC 18
pa_status pa_copy_kernel_kind_soa(int nd, const int64_t *dims,
                                  const int64_t *sstr, int64_t soff,
                                  const int64_t *dstr, int64_t doff,
                                  int64_t scalar_size, int n, int dir,
                                  const void *aos, const void *const *fields,
                                  int64_t out[5]);

/* ---- zero fill (truncated transposes) ---------------------------------- */
/* Zero one destination-only window on the device (the kernel body a keep
 * plan's grouped fill runs): dst[doff + sum j_i*dstr_i] = 0 for j over dims,
 * in elements of scalar_size * ncomp bytes.  An empty window launches
 * nothing.  dst must be aligned to its scalar. */
pa_status pa_device_fill_zero(int nd, const int64_t *dims,
                              const int64_t *dstr, int64_t doff,
                              int64_t scalar_size, int64_t ncomp, void *dst,
                              void *stream);
/* Which stores the fill makes (host-only; dst is used for its alignment
 * only).  out = {kind, store_bytes}: PA_KERNEL_FILL, or PA_KERNEL_NONE with
 * 0 for an empty window.  store_bytes is the widest of 16, 8, 4 that divides
 * the base pointer, the offset and every non-unit stride in bytes, and the
 * run length in bytes (a window contiguous along its fastest axis, one lane
 * per store) or the element size (any other window, one lane per element);
 * else 1. */
#define PA_KERNEL_FILL 12
pa_status pa_fill_kernel_kind(int nd, const int64_t *dims,
                              const int64_t *dstr, int64_t doff,
                              int64_t scalar_size, int64_t ncomp,
                              const void *dst, int64_t out[2]);

#ifdef __cplusplus
}
#endif

#endif /* PENCILHIP_H */
