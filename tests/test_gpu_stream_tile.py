"""GPU tests for the streaming form of the 8-byte vector-store tile
(k_transpose_tile_vs_nt: nontemporal loads and nontemporal 16-byte vector
stores), which select_kernel() picks from 512 MiB of payload up.

The threshold is forced to 0 (and restored afterwards), so the small
boundary shapes of test_gpu_word_tiles.py run the streaming kernels.  Every
case runs through pa_device_copy, asserts that pa_copy_kernel_stream reports
streaming and that pa_copy_kernel_kind reports what it reports without it,
and compares the WHOLE 0xAB-prefilled destination (slack included) bit for
bit with the CPU executor apply_copy, or with a numpy transpose where that
is too slow.  The reference is never another device run.
"""

import numpy as np
import pytest

import oracle as orc
from pencilarrays_amd import Pencil, PencilArray, Topology, Transposition
from pencilarrays_amd.copyexec import apply_copy

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from pencilarrays_amd import native  # noqa: E402
from tile_util import (  # noqa: E402
    NP_BITS, dev_copy, extent, kernel_of, rand_bits, same_bytes, sentinel_gpu,
    sentinel_np, to_gpu, to_np, transpose_desc,
)

TILE, TILE_VS = native.KERNEL_TILE, native.KERNEL_TILE_VS
NB = 3
SLACK = 4  # elements after the last one written: a spill lands in-buffer
VS_N0 = [2, 63, 64, 65, 2 * 64 + 3]
VS_NTA = [2, 3, 127, 128, 129, 2 * 128 + 3]


@pytest.fixture
def stream_always():
    old = native.set_stream_min_bytes(0)
    try:
        yield
    finally:
        native.set_stream_min_bytes(old)


def _stream_of(desc, src_t, dst_t):
    return native.copy_kernel_stream(desc, 8, src_t.data_ptr(),
                                     dst_t.data_ptr())


def _run(desc, src, dst_n, want, stream, exp=None):
    """pa_device_copy of ``desc`` into a sentinel-filled destination; kind
    and policy asserted BEFORE the copy runs, the whole destination compared
    with ``exp`` (default: apply_copy on a sentinel-filled buffer)."""
    if exp is None:
        exp = sentinel_np(dst_n, 8)
        apply_copy(desc, src, exp)
    assert extent(desc, desc.sstrides, desc.soffset) <= src.size
    assert extent(desc, desc.dstrides, desc.doffset) <= dst_n == exp.size
    src_t = to_gpu(src)
    dst_t = sentinel_gpu(dst_n, 8)
    k = kernel_of(desc, 8, src_t, dst_t)
    what = f"{desc} kind={k}"
    assert (k.kind, k.word_bytes, k.byteified, k.sweep_depth) == want, what
    # the kind query is what it is with streaming switched off
    off = native.set_stream_min_bytes(-1)
    try:
        assert kernel_of(desc, 8, src_t, dst_t) == k, what
        assert _stream_of(desc, src_t, dst_t) == 0, what
    finally:
        native.set_stream_min_bytes(off)
    assert _stream_of(desc, src_t, dst_t) == stream, what
    dev_copy(desc, 8, src_t, dst_t)
    torch.cuda.synchronize()
    assert same_bytes(to_np(dst_t, 8), exp), what


def _boundary(rng, n0, nta, dense):
    if dense:
        sp, so, dp, do = n0, 0, nta, 0
    else:
        sp, so, dp, do = n0 + 4 + (n0 & 1), 6, nta + 2 + (nta & 1), 4
    desc = transpose_desc(n0, nta, NB, sp, so, dp, do)
    src = rand_bits(rng, extent(desc, desc.sstrides, so), 8)
    return desc, src, extent(desc, desc.dstrides, do) + SLACK


def test_streaming_boundary_shapes_windows(stream_always):
    """5 x 6 extents around the 64 x 128 tile edges, windows with even
    pitches and offsets: every case streams.  Odd nta takes the plain scalar
    tail element next to the nontemporal vector stores."""
    rng = np.random.default_rng(2108)
    for n0 in VS_N0:
        for nta in VS_NTA:
            desc, src, dst_n = _boundary(rng, n0, nta, dense=False)
            _run(desc, src, dst_n, (TILE_VS, 8, 0, 1), 1)


def test_streaming_boundary_shapes_dense(stream_always):
    """Dense buffers: even nta stream; a dense row of odd nta has an odd
    pitch, runs the scalar tile and reports no streaming."""
    rng = np.random.default_rng(2208)
    for n0 in VS_N0:
        for nta in VS_NTA:
            desc, src, dst_n = _boundary(rng, n0, nta, dense=True)
            odd = nta & 1
            _run(desc, src, dst_n, (TILE if odd else TILE_VS, 8, 0, 1),
                 0 if odd else 1)


def test_default_threshold_small_shapes_do_not_stream():
    """No threshold forced: the same shapes report the plain policy."""
    rng = np.random.default_rng(2308)
    assert native.set_stream_min_bytes(512 << 20) == 512 << 20
    for dense in (False, True):
        for n0 in VS_N0:
            for nta in VS_NTA:
                desc, _, _ = _boundary(rng, n0, nta, dense)
                assert native.copy_kernel_stream(desc, 8, 0, 0) == 0, desc


# (n0, nta, nb, depth): 67 or 259 tiles along ta, so the last chunk is short
# (takes the break) and the last tile is partial with an odd tail; the
# shapes of test_gpu_word_tiles.py's ragged sweeps (68 and 269 MB).
RAGGED = {
    "d8": (2, 66 * 128 + 37, 497, 8),
    "d32": (2, 258 * 128 + 37, 509, 32),
}


@pytest.mark.parametrize("case", sorted(RAGGED))
def test_streaming_ragged_sweep(case, stream_always):
    """The streaming kernels of sweep depth 8 and 32: the JCHUNK loop with
    its break and the barrier between tiles.  Expectation by numpy
    transpose."""
    n0, nta, nb, depth = RAGGED[case]
    assert -(-nta // 128) % depth and nta % 128, "shape must stay ragged"
    pitch = nta + 1
    desc = transpose_desc(n0, nta, nb, n0, 0, pitch, 0)
    rng = np.random.default_rng(2600)
    src = rng.integers(0, 2 ** 64, n0 * nta * nb, dtype=NP_BITS[8],
                       endpoint=False)
    dst_n = pitch * n0 * nb + SLACK
    exp = sentinel_np(dst_n, 8)
    exp[:pitch * n0 * nb].reshape(nb, n0, pitch)[:, :, :nta] = \
        src.reshape(nb, nta, n0).transpose(0, 2, 1)
    try:
        _run(desc, src, dst_n, (TILE_VS, 8, 0, depth), 1, exp=exp)
    finally:
        del src, exp
        torch.cuda.empty_cache()


def test_streaming_aliased_round_trip_through_a_plan(stream_always):
    """x -> y -> x in place through pa_transpose_execute with the threshold
    at 0: the forward plan's transposing entry has sweep depth 8, so it is
    launched on its own (not grouped) on the streaming kernel, reading the
    staged copy the aliased plan made on the same stream.  Bit-identical to
    the CPU oracle both ways."""
    dims = (2, 1026, 4100)  # 32865 tiles along ta: short last chunk
    topo = Topology((1, 1))
    p1 = Pencil(topo, dims, (1, 2))
    p2 = Pencil(topo, dims, (0, 2), permute=(1, 2, 0))
    n = p1.length_local(0)
    assert n == p2.length_local(0)
    buf = torch.empty(n, dtype=torch.float64, device="cuda:0")
    src_np = np.random.default_rng(2700).standard_normal(n)
    buf.copy_(torch.from_numpy(src_np))
    src = PencilArray(p1, 0, buf)
    dst = PencilArray(p2, 0, buf)
    t = Transposition(dst, src)
    assert t.aliased
    t.execute()
    torch.cuda.synchronize()

    plan = t._native.native
    streamed = []
    for which in range(5):
        desc = plan.copydesc(which)
        if desc is None:
            continue
        k = native.copy_kernel_kind(desc, 8)
        if k.kind == TILE_VS and k.sweep_depth > 1:
            streamed.append(native.copy_kernel_stream(desc, 8))
    assert streamed and all(streamed), streamed
    launches = [l for st in (native.STAGE_PACK, native.STAGE_LOCAL)
                for l in plan.stage_launches(1, st)]
    assert any(l.kind == TILE_VS and not l.grouped for l in launches), launches

    exp = orc.transpose_oracle([src_np], dims, (1, 1), (1, 2), (0, 1, 2),
                               (0, 2), (1, 2, 0), ())[0]
    assert np.array_equal(dst.data.cpu().numpy(), exp)
    t2 = Transposition(src, dst)
    assert t2.aliased
    t2.execute()
    torch.cuda.synchronize()
    assert np.array_equal(src.data.cpu().numpy(), src_np)
