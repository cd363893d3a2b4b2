"""Cache policy of the vector-store tile (pa_copy_kernel_stream,
pa_set_stream_min_bytes): host-only, like test_kernel_select.py.

- the policy flips exactly at the threshold, in payload bytes of one
  direction, and the kind query does not depend on it;
- every kind other than TILE_VS reports 0, whatever the threshold;
- pa_set_stream_min_bytes returns the previous value; 0 streams wherever the
  tile runs, a negative value never.
"""

import os

import pytest

native = pytest.importorskip("pencilarrays_amd.native")

if not os.path.exists(native.lib_path()):
    pytest.skip("libpencilhip.so not built", allow_module_level=True)

PTR = 0x7F0000000000  # fake, 256-byte aligned, never dereferenced
QPTR = 0x7F0000100000
DEFAULT_MIN = 512 << 20


@pytest.fixture
def threshold():
    """Set the threshold for one test; the default is back afterwards."""
    first = []

    def set_(v):
        old = native.set_stream_min_bytes(v)
        if not first:
            first.append(old)
        return old

    try:
        yield set_
    finally:
        if first:
            native.set_stream_min_bytes(first[0])


def transpose2d(n0, nta, d_pitch=None, doff=0):
    """src[i + n0*j] -> dst[doff + j + d_pitch*i]"""
    return ((n0, nta), (1, n0), 0, (d_pitch or nta, 1), doff)


def both(desc, esz=8, sp=PTR, dp=QPTR):
    return (native.copy_kernel_kind(desc, esz, sp, dp),
            native.copy_kernel_stream(desc, esz, sp, dp))


def test_default_threshold_is_512_mib(threshold):
    assert threshold(DEFAULT_MIN) == DEFAULT_MIN


def test_flips_exactly_at_the_default_threshold():
    """2 x (2^25 - 1) elements are one element pair short of 512 MiB."""
    below = transpose2d(2, (1 << 25) - 1, d_pitch=1 << 25)
    at = transpose2d(2, 1 << 25)
    assert 2 * ((1 << 25) - 1) * 8 == DEFAULT_MIN - 16
    kb, sb = both(below)
    ka, sa = both(at)
    assert kb.kind == ka.kind == native.KERNEL_TILE_VS
    assert (sb, sa) == (0, 1)
    # the same shape in 8 MiB-pitch rows, the headline descriptor
    k, s = both(transpose2d(1024, 1 << 20))
    assert (k.kind, k.sweep_depth, s) == (native.KERNEL_TILE_VS, 32, 1)


def test_flips_exactly_at_a_set_threshold(threshold):
    threshold(64 * 130 * 8)
    below = transpose2d(64, 129, d_pitch=130)
    pair = transpose2d(2, 32 * 130 - 1, d_pitch=32 * 130)    # 2 elements short
    at = transpose2d(64, 130)
    for desc, want in [(below, 0), (pair, 0), (at, 1)]:
        k, s = both(desc)
        assert k.kind == native.KERNEL_TILE_VS, desc
        assert s == want, desc


def test_kind_query_does_not_depend_on_the_threshold(threshold):
    descs = [transpose2d(64, 130), transpose2d(1024, 1 << 20),
             transpose2d(2, 66 * 128 + 38)]
    before = [native.copy_kernel_kind(d, 8, PTR, QPTR) for d in descs]
    for v, want in [(0, 1), (-1, 0), (1 << 62, 0)]:
        threshold(v)
        for d, kb in zip(descs, before):
            k, s = both(d)
            assert k == kb and s == want, (v, d)


N = 64
OTHER_KINDS = {
    # name: (descriptor, elem size, dst pointer, kind it must select)
    "tile8_odd_doff": (transpose2d(N, 130, doff=1), 8, QPTR,
                       native.KERNEL_TILE),
    "tile8_misaligned_dst": (transpose2d(N, 130), 8, QPTR + 8,
                             native.KERNEL_TILE),
    "tile8_odd_pitch": (transpose2d(N, 129), 8, QPTR, native.KERNEL_TILE),
    "tile4": (transpose2d(N, 130), 4, QPTR, native.KERNEL_TILE),
    "tile16": (transpose2d(N, 130), 16, QPTR, native.KERNEL_TILE),
    "tile_pk": (transpose2d(N, 136), 2, QPTR, native.KERNEL_TILE_PK),
    "copy_1d": (((4096,), (1,), 0, (1,), 0), 8, QPTR, native.KERNEL_COPY_1D),
    "copy_1d_nt": (((1 << 27,), (1,), 0, (1,), 0), 8, QPTR,
                   native.KERNEL_COPY_1D_NT),
    "linear": (((N, N), (1, N + 2), 0, (1, N + 4), 0), 8, QPTR,
               native.KERNEL_LINEAR),
    "generic": (((N, N), (2, 2 * N), 0, (2 * N, 2), 0), 8, QPTR,
                native.KERNEL_GENERIC),
    "byteified": (transpose2d(N, 130), 3, QPTR, native.KERNEL_LINEAR),
    "empty": (((0,), (1,), 0, (1,), 0), 8, QPTR, native.KERNEL_NONE),
}


@pytest.mark.parametrize("name", sorted(OTHER_KINDS))
def test_every_other_kind_reports_zero(name, threshold):
    desc, esz, dp, kind = OTHER_KINDS[name]
    threshold(0)
    k, s = both(desc, esz, dp=dp)
    assert k.kind == kind, k
    assert s == 0
    # the control: the vector-store tile does stream at threshold 0
    assert both(transpose2d(N, 130))[1] == 1


def test_set_returns_the_previous_value(threshold):
    assert threshold(12345) == DEFAULT_MIN
    assert threshold(0) == 12345
    assert threshold(-1) == 0
    assert threshold(DEFAULT_MIN) == -1
