"""Kernel selection for composite elements (pa_copy_kernel_kind_comp): an
element of ``ncomp`` scalars of ``scalar_size`` bytes, components fastest.

Host-only, like test_kernel_select.py whose 64^3 transposed descriptor and
fake pointers this file reuses.  With B = scalar_size * ncomp:

- ncomp = 1 is exactly the plain elem_size decision;
- B in {1,2,4,8,16} reuses the tuned kernels of elem_size = B;
- transposable descriptors with B <= 64 take the wide tile in W-byte words,
  W = largest power of two <= 16 dividing B and both base addresses, with
  m = B / W words per element;
- everything else runs the linear kernel on the word-expanded descriptor,
  never the byte-ify fallback.
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
T_DIMS = (N, N, N)
T_SSTR = (1, N, N * N)
T_DSTR = (N * N, 1, N)
NOCONT_SSTR = (2, 2 * N, 2 * N * N)


def kind(dims, sstr, soff, dstr, doff, ssz, ncomp, sp=PTR, dp=QPTR):
    return native.copy_kernel_kind((dims, sstr, soff, dstr, doff), ssz, sp,
                                   dp, ncomp=ncomp)


def transposed(ssz, ncomp, sp=PTR, dp=QPTR, **kw):
    return kind(T_DIMS, kw.get("sstr", T_SSTR), kw.get("soff", 0),
                kw.get("dstr", T_DSTR), kw.get("doff", 0), ssz, ncomp, sp, dp)


# ---- ncomp = 1: the old query ---------------------------------------------

# one descriptor of every class test_kernel_select.py uses
CLASSES = {
    "transposed": (T_DIMS, T_SSTR, 0, T_DSTR, 0),
    "transposed_odd_doff": (T_DIMS, T_SSTR, 0, T_DSTR, 1),
    "transposed_odd_soff": (T_DIMS, T_SSTR, 1, T_DSTR, 0),
    "sweep8": ((1024, 64 * 64, 64), (1, 1024, 1024 * 64 * 64), 0,
               (64 * 64 * 64, 1, 64 * 64), 1),
    "contiguous": (T_DIMS, T_SSTR, 0, T_SSTR, 0),
    "contiguous_large": (((512 << 20) // 8,), (1,), 0, (1,), 0),
    "linear_window": ((32, 16), (1, 40), 0, (1, 32), 0),
    "linear_odd_run": ((33, 16), (1, 41), 0, (1, 33), 0),
    "no_contiguous_axis": (T_DIMS, NOCONT_SSTR, 0, T_DSTR, 0),
    "empty": ((0, 4), (1, 4), 0, (4, 1), 0),
}


@pytest.mark.parametrize("esz", [1, 2, 3, 4, 6, 8, 12, 16, 24])
@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("ptrs", [(PTR, QPTR), (PTR + 8, QPTR + 8)])
def test_ncomp1_equals_plain_query(cls, esz, ptrs):
    desc = CLASSES[cls]
    old = native.copy_kernel_kind(desc, esz, *ptrs)
    lib = native.load()
    dims, sstr, soff, dstr, doff = desc
    nd = len(dims)
    I64 = native.I64
    out = (I64 * 5)()
    st = lib.pa_copy_kernel_kind_comp(
        nd, (I64 * nd)(*dims), (I64 * nd)(*sstr), I64(soff),
        (I64 * nd)(*dstr), I64(doff), I64(esz), I64(1),
        native.VP(ptrs[0]), native.VP(ptrs[1]), out)
    assert st == 0, lib.pa_last_error().decode()
    assert tuple(out)[:4] == tuple(old)[:4]
    assert out[4] == 1


# ---- wide tile --------------------------------------------------------------

WIDE = [(8, 3, 8, 3), (4, 3, 4, 3), (2, 3, 2, 3), (1, 3, 1, 3),
        (16, 3, 16, 3), (16, 2, 16, 2), (4, 6, 8, 3), (8, 6, 16, 3),
        (4, 5, 4, 5), (1, 7, 1, 7), (8, 8, 16, 4)]


@pytest.mark.parametrize("ssz,ncomp,W,m", WIDE)
def test_wide_tile_word_and_count(ssz, ncomp, W, m):
    k = transposed(ssz, ncomp)
    assert (k.kind, k.word_bytes, k.byteified, k.words_per_element) == \
        (native.KERNEL_TILE_WIDE, W, 0, m)
    assert native.KERNEL_NAMES[k.kind] == "TILE_WIDE"


@pytest.mark.parametrize("ssz,ncomp,want", [
    (4, 2, (native.KERNEL_TILE_VS, 8)),
    (8, 2, (native.KERNEL_TILE, 16)),
    (4, 4, (native.KERNEL_TILE, 16)),
    (2, 2, (native.KERNEL_TILE, 4)),
    (1, 2, (native.KERNEL_TILE_PK, 2)),
])
def test_power_of_two_totals_reuse_tuned_kernels(ssz, ncomp, want):
    k = transposed(ssz, ncomp)
    assert (k.kind, k.word_bytes) == want
    assert k.byteified == 0
    # the very decision of elem_size = B
    assert tuple(k)[:4] == tuple(native.copy_kernel_kind(
        (T_DIMS, T_SSTR, 0, T_DSTR, 0), ssz * ncomp, PTR, QPTR))[:4]


def test_misaligned_base_pointers_lower_the_word():
    k = transposed(4, 6, sp=PTR + 4)
    assert (k.kind, k.word_bytes, k.words_per_element) == \
        (native.KERNEL_TILE_WIDE, 4, 6)
    k = transposed(8, 6, dp=QPTR + 8)
    assert (k.kind, k.word_bytes, k.words_per_element) == \
        (native.KERNEL_TILE_WIDE, 8, 6)


def test_elements_past_64_bytes_take_word_expanded_linear():
    k = transposed(8, 9)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_LINEAR, 8, 0)
    assert k.words_per_element == 9
    k = transposed(16, 5)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_LINEAR, 16, 0)
    # 64 bytes is still inside the cap
    assert transposed(16, 4).kind == native.KERNEL_TILE_WIDE


def test_linear_at_element_level():
    k = kind(T_DIMS, T_SSTR, 0, T_SSTR, 0, 8, 3)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_COPY_1D, 16, 0)
    k = kind((33, 16), (1, 41), 0, (1, 33), 0, 4, 3)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_LINEAR, 4, 0)
    # a base address that is only 8-byte aligned caps the word
    k = kind(T_DIMS, T_SSTR, 0, T_SSTR, 0, 8, 3, dp=QPTR + 8)
    assert (k.kind, k.word_bytes) == (native.KERNEL_COPY_1D, 8)


def test_no_contiguous_axis_is_word_expanded_linear():
    k = kind(T_DIMS, NOCONT_SSTR, 0, T_DSTR, 0, 8, 3)
    assert (k.kind, k.word_bytes, k.byteified) == (native.KERNEL_LINEAR, 8, 0)


def test_invalid_pairs_are_errors_with_a_message():
    with pytest.raises(RuntimeError, match="scalar_size"):
        transposed(3, 2)
    with pytest.raises(RuntimeError, match="ncomp"):
        transposed(8, 0)
    topo = Topology((1, 1))
    P = Pencil(topo, (8, 8, 8), (1, 2))
    with pytest.raises(RuntimeError, match="scalar_size"):
        native.NativePlan(P, P, 0, 3, ncomp=2)
    with pytest.raises(RuntimeError, match="ncomp"):
        native.NativePlan(P, P, 0, 8, ncomp=0)


# ---- plan level -------------------------------------------------------------

def test_world1_permuted_plan_local_copy_is_wide_tile():
    dims = (64, 64, 64)
    topo = Topology((1, 1))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    plan = native.NativePlan(Pi, Po, 0, 8, ncomp=3)
    desc = plan.copydesc(0)
    assert desc is not None
    # element units: the same descriptor as the scalar plan
    assert desc == native.NativePlan(Pi, Po, 0, 8).copydesc(0)
    k = native.copy_kernel_kind(desc, 8, PTR, QPTR, ncomp=3)
    assert native.KERNEL_NAMES[k.kind] == "TILE_WIDE"
    assert (k.word_bytes, k.words_per_element, k.byteified) == (8, 3, 0)


def test_buffer_sizes_carry_the_element_bytes():
    dims = (16, 21, 41)
    topo = Topology((2, 2))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    for rank in range(4):
        s1, r1 = native.NativePlan(Pi, Po, rank, 1).buffer_sizes()
        s, r = native.NativePlan(Pi, Po, rank, 8, ncomp=3).buffer_sizes()
        assert s1 > 0 and r1 > 0
        assert (s, r) == (s1 * 24, r1 * 24)
