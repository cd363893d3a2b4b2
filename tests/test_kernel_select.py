"""Kernel selection (pa_copy_kernel_kind): which kernel a descriptor runs.

Host-only: the query needs the built library but no GPU, and the pointer
arguments are fake addresses used for their alignment only.  The launcher
executes exactly the decision the query reports (one decision function in
the engine), so these pins describe pa_device_copy and pa_transpose_execute.

- element sizes 4/8/16 keep the dispatch they had before the query existed;
- 1-/2-byte elements: packed tile when every 8-byte access is aligned, the
  scalar tile for each single misalignment, the generic kernel without a
  contiguous axis, never the byte-ify fallback;
- composite sizes (3, 6, 12) still byte-ify.
"""

import os

import pytest

from pencilarrays_amd import Pencil, Topology

native = pytest.importorskip("pencilarrays_amd.native")

if not os.path.exists(native.lib_path()):
    pytest.skip("libpencilhip.so not built", allow_module_level=True)

PTR = 0x7F0000000000  # fake, 256-byte aligned, never dereferenced
QPTR = 0x7F0000100000

N = 64
# src axis 0 fastest; dst fastest along axis 1, then axis 2, then axis 0
T_DIMS = (N, N, N)
T_SSTR = (1, N, N * N)
T_DSTR = (N * N, 1, N)


def kind(dims, sstr, soff, dstr, doff, esz, sp=PTR, dp=QPTR):
    return native.copy_kernel_kind((dims, sstr, soff, dstr, doff), esz, sp, dp)


def transposed(esz, soff=0, doff=0, sstr=T_SSTR, dstr=T_DSTR, sp=PTR, dp=QPTR):
    return kind(T_DIMS, sstr, soff, dstr, doff, esz, sp, dp)


# ---- 1. existing sizes: today's dispatch ---------------------------------

def test_esz8_even_takes_vector_store_tile():
    k = transposed(8)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_TILE_VS, 8, 0)
    assert k.sweep_depth == 1


def test_esz8_odd_doff_takes_scalar_tile():
    k = transposed(8, doff=1)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_TILE, 8, 0)


def test_esz8_misaligned_dst_pointer_takes_scalar_tile():
    k = transposed(8, dp=QPTR + 8)
    assert (k.kind, k.word_bytes) == (native.KERNEL_TILE, 8)


@pytest.mark.parametrize("esz", [4, 16])
def test_esz4_and_16_take_scalar_tile(esz):
    k = transposed(esz)
    assert (k.kind, k.word_bytes, k.byteified, k.sweep_depth) == \
        (native.KERNEL_TILE, esz, 0, 1)


@pytest.mark.parametrize("esz", [4, 8])
def test_sweep_depth_thresholds(esz):
    """8 x ntj x 64 tiles of the 128x64 scalar tile (odd doff keeps esz 8
    off the vector-store tile): ntj = 64 -> depth 8, ntj = 256 -> 32."""
    for n_ta, depth in [(64 * 64, 8), (256 * 64, 32), (63 * 64, 1)]:
        dims = (1024, n_ta, 64)
        sstr = (1, 1024, 1024 * n_ta)
        dstr = (n_ta * 64, 1, n_ta)
        k = kind(dims, sstr, 0, dstr, 1, esz)
        assert (k.kind, k.sweep_depth) == (native.KERNEL_TILE, depth)
    # the vector-store tile is 64x128: 16 x 256 x 64 tiles -> depth 32
    if esz == 8:
        n_ta = 256 * 128
        k = kind((1024, n_ta, 64), (1, 1024, 1024 * n_ta),
                 0, (n_ta * 64, 1, n_ta), 0, 8)
        assert (k.kind, k.sweep_depth) == (native.KERNEL_TILE_VS, 32)


def test_contiguous_takes_copy_1d():
    k = kind(T_DIMS, T_SSTR, 0, T_SSTR, 0, 8)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_COPY_1D, 16, 0)


def test_contiguous_large_takes_nontemporal_copy():
    n = (512 << 20) // 8
    k = kind((n,), (1,), 0, (1,), 0, 8)
    assert (k.kind, k.word_bytes) == (native.KERNEL_COPY_1D_NT, 16)
    k = kind((n - 2,), (1,), 0, (1,), 0, 8)
    assert (k.kind, k.word_bytes) == (native.KERNEL_COPY_1D, 16)


def test_linear_runs_window():
    k = kind((32, 16), (1, 40), 0, (1, 32), 0, 8)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_LINEAR, 16, 0)
    # odd run length: 8-byte words
    k = kind((33, 16), (1, 41), 0, (1, 33), 0, 8)
    assert (k.kind, k.word_bytes) == (native.KERNEL_LINEAR, 8)


def test_no_contiguous_axis_esz8_is_generic():
    k = kind(T_DIMS, (2, 2 * N, 2 * N * N), 0, T_DSTR, 0, 8)
    assert (k.kind, k.word_bytes) == (native.KERNEL_GENERIC, 8)


def test_empty_descriptor():
    k = kind((0, 4), (1, 4), 0, (4, 1), 0, 8)
    assert k.kind == native.KERNEL_NONE


# ---- 2. 1- and 2-byte elements -------------------------------------------

@pytest.mark.parametrize("esz", [1, 2])
def test_small_aligned_takes_packed_tile(esz):
    k = transposed(esz)
    assert (k.kind, k.word_bytes, k.byteified, k.sweep_depth) == \
        (native.KERNEL_TILE_PK, esz, 0, 1)


MISALIGN = {
    "odd_soff": dict(soff=1),
    "odd_doff": dict(doff=1),
    "odd_outer_sstr": dict(sstr=(1, N, N * N + 1)),
    "odd_ta_sstr": dict(sstr=(1, N + 1, (N + 1) * N)),
    "odd_outer_dstr": dict(dstr=(N * N, 1, N + 1)),
    "odd_axis0_dstr": dict(dstr=(N * N + 1, 1, N)),
    "src_ptr_plus_esz": "sp",
    "dst_ptr_plus_esz": "dp",
}


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("what", sorted(MISALIGN))
def test_small_each_misalignment_alone_takes_scalar_tile(esz, what):
    """The packed tile needs BOTH sides aligned (one fast-path flag): any
    single misalignment selects the scalar tile in esz-byte words."""
    kw = MISALIGN[what]
    if kw == "sp":
        kw = dict(sp=PTR + esz)
    elif kw == "dp":
        kw = dict(dp=QPTR + esz)
    k = transposed(esz, **kw)
    assert (k.kind, k.word_bytes, k.byteified, k.sweep_depth) == \
        (native.KERNEL_TILE, esz, 0, 1)


@pytest.mark.parametrize("esz", [1, 2])
def test_small_vector_multiple_offsets_stay_packed(esz):
    v = 8 // esz
    k = transposed(esz, soff=v, doff=3 * v, sp=PTR + 8, dp=QPTR + 24)
    assert k.kind == native.KERNEL_TILE_PK
    # a multiple of half a vector is not enough
    k = transposed(esz, soff=v // 2)
    assert k.kind == native.KERNEL_TILE


@pytest.mark.parametrize("esz", [1, 2])
def test_small_no_contiguous_axis_is_generic(esz):
    k = kind(T_DIMS, (2, 2 * N, 2 * N * N), 0, T_DSTR, 0, esz)
    assert (k.kind, k.word_bytes, k.byteified) == \
        (native.KERNEL_GENERIC, esz, 0)


def test_linear_esz2_is_word_scaled_as_before():
    k = kind(T_DIMS, T_SSTR, 0, T_SSTR, 0, 2)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_COPY_1D, 16, 0)
    k = kind((32, 16), (1, 40), 0, (1, 32), 0, 2)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_LINEAR, 16, 0)
    k = kind((34, 16), (1, 42), 0, (1, 34), 0, 2)
    assert (k.kind, k.word_bytes) == (native.KERNEL_LINEAR, 4)
    # 66-byte runs: no word fits, byte words (not the byte-ify fallback)
    k = kind((33, 16), (1, 41), 0, (1, 33), 0, 2)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_LINEAR, 1, 0)


# ---- 3. composite element sizes still byte-ify ----------------------------

@pytest.mark.parametrize("esz,word", [(3, 1), (6, 1), (12, 4), (24, 8)])
def test_composite_sizes_still_byteify(esz, word):
    k = transposed(esz)
    assert (k.kind, k.word_bytes, k.byteified) == \
        (native.KERNEL_LINEAR, word, 1)


# ---- 4. plan level ---------------------------------------------------------

@pytest.mark.parametrize("esz,want", [(2, "TILE_PK"), (1, "TILE_PK"),
                                      (8, "TILE_VS"), (4, "TILE")])
def test_world1_permuted_plan_local_copy(esz, want):
    dims = (64, 64, 64)
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    plan = native.NativePlan(Pi, Po, 0, esz)
    desc = plan.copydesc(0)
    assert desc is not None
    k = native.copy_kernel_kind(desc, esz, PTR, QPTR)
    assert native.KERNEL_NAMES[k.kind] == want
    assert (k.word_bytes, k.byteified) == (esz, 0)


def test_accepts_copydesc_objects():
    from pencilarrays_amd.plan import CopyDesc
    d = CopyDesc(dims=T_DIMS, sstrides=T_SSTR, soffset=0,
                 dstrides=T_DSTR, doffset=0)
    assert native.copy_kernel_kind(d, 2, PTR, QPTR).kind == \
        native.KERNEL_TILE_PK
    # default pointers (0) count as aligned
    assert native.copy_kernel_kind(d, 2).kind == native.KERNEL_TILE_PK


# ---- 5. the linear path honours base-pointer alignment ---------------------

def _widest_word(run_bytes, *addrs):
    """The rule, restated: the widest of {16, 8, 4, 1} bytes that divides
    the run and every address."""
    for w in (16, 8, 4, 1):
        if run_bytes % w == 0 and all(a % w == 0 for a in addrs):
            return w


SHIFTS = {"src": (1, 0), "dst": (0, 1), "both": (1, 1)}


@pytest.mark.parametrize("esz", [1, 2, 4, 8])
@pytest.mark.parametrize("which", sorted(SHIFTS))
def test_contiguous_copy_word_divides_shifted_pointers(esz, which):
    """A contiguous run whose base pointer is moved by one element (a sliced
    tensor) on the src side, the dst side, and both."""
    ss, ds = SHIFTS[which]
    sp, dp = PTR + ss * esz, QPTR + ds * esz
    n = 4096
    k = kind((n,), (1,), 0, (1,), 0, esz, sp, dp)
    assert (k.kind, k.byteified) == (native.KERNEL_COPY_1D, 0)
    assert sp % k.word_bytes == 0 and dp % k.word_bytes == 0, k
    assert k.word_bytes == _widest_word(n * esz, sp, dp), k
    # the unshifted copy keeps 16-byte words
    k = kind((n,), (1,), 0, (1,), 0, esz)
    assert (k.kind, k.word_bytes) == (native.KERNEL_COPY_1D, 16)


@pytest.mark.parametrize("esz", [1, 2, 4, 8])
@pytest.mark.parametrize("which", sorted(SHIFTS))
def test_linear_window_word_divides_shifted_pointers(esz, which):
    """A two-axis linear window (runs of 64 elements, 16-byte-multiple
    pitches and offsets) from pointers moved by one element."""
    ss, ds = SHIFTS[which]
    sp, dp = PTR + ss * esz, QPTR + ds * esz
    desc = ((64, 16), (1, 96), 32, (1, 80), 16)
    k = kind(*desc, esz, sp, dp)
    assert (k.kind, k.byteified) == (native.KERNEL_LINEAR, 0)
    assert sp % k.word_bytes == 0 and dp % k.word_bytes == 0, k
    assert k.word_bytes == _widest_word(64 * esz, sp, dp), k
    k = kind(*desc, esz)
    assert (k.kind, k.word_bytes) == (native.KERNEL_LINEAR, 16)


def test_shifted_pointer_words_issue_examples():
    k = kind((4096,), (1,), 0, (1,), 0, 1, PTR + 1, QPTR + 3)
    assert (k.kind, k.word_bytes) == (native.KERNEL_COPY_1D, 1)
    k = kind((4096,), (1,), 0, (1,), 0, 2, PTR + 2, QPTR)
    assert (k.kind, k.word_bytes) == (native.KERNEL_COPY_1D, 1)
    k = kind((32, 16), (1, 40), 0, (1, 32), 0, 8, PTR + 8, QPTR)
    assert (k.kind, k.word_bytes) == (native.KERNEL_LINEAR, 8)
    # a pointer that is a multiple of 16 but not of 256 changes nothing
    k = kind((32, 16), (1, 40), 0, (1, 32), 0, 8, PTR + 16, QPTR + 48)
    assert (k.kind, k.word_bytes) == (native.KERNEL_LINEAR, 16)


@pytest.mark.parametrize("which", sorted(SHIFTS))
def test_large_copy_from_8mod16_pointer_is_not_nontemporal(which):
    """The nontemporal copy moves 16-byte words: >= 512 MiB from or to a
    pointer that is 8 mod 16 takes the plain copy in 8-byte words."""
    ss, ds = SHIFTS[which]
    n = (512 << 20) // 8
    k = kind((n,), (1,), 0, (1,), 0, 8, PTR + 8 * ss, QPTR + 8 * ds)
    assert (k.kind, k.word_bytes) == (native.KERNEL_COPY_1D, 8)
