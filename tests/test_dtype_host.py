"""Half-precision / 8-bit element types on the host side (no GPU):

- gather_sim on torch.bfloat16 arrays returns the uint16 bit patterns, placed
  exactly as int16 data is (numpy has no bfloat16);
- gather_sim on float16 is unchanged (a real numpy float16 array);
- the MPI-IO driver rejects bfloat16 with its own "unsupported element type"
  error, on write and on read, without touching the file;
- PencilArray.empty / ManyPencilArray pick torch storage when a device is
  given, for every small dtype.
"""

import numpy as np
import pytest

from pencilarrays_amd import (
    ManyPencilArray, Pencil, PencilArray, Topology, gather_sim,
)
from pencilarrays_amd.dtypes import bits_dtype, numpy_dtype, to_numpy
from pencilarrays_amd.pencilio import MPIIOFile

torch = pytest.importorskip("torch")

DIMS = (6, 7, 5)
PDIMS = (2, 2)


def _arrays(dtype, permute=(1, 2, 0)):
    """One PencilArray per rank holding seeded int16 bit patterns viewed as
    ``dtype`` (a 2-byte torch dtype), plus the int16 twins."""
    topo = Topology(PDIMS)
    p = Pencil(topo, DIMS, (0, 2), permute=permute)
    rng = np.random.default_rng(7)
    xs, twins = [], []
    for r in range(topo.nranks):
        bits = rng.integers(-2**15, 2**15, p.length_local(r), dtype=np.int16)
        t = torch.from_numpy(bits.copy())
        xs.append(PencilArray(p, r, t.view(dtype)))
        twins.append(PencilArray(p, r, t.clone()))
    return xs, twins


def test_gather_sim_bfloat16_returns_uint16_bit_patterns():
    xs, twins = _arrays(torch.bfloat16)
    got = gather_sim(xs)
    ref = gather_sim(twins)  # int16 path, unchanged code
    assert got.dtype == np.uint16
    assert ref.dtype == np.int16
    assert got.shape == DIMS
    assert np.array_equal(got, ref.view(np.uint16))


def test_gather_sim_bfloat16_values_round_trip():
    """The bit patterns are the bfloat16 values: widening them back gives the
    tensors' float32 values at the same global positions."""
    xs, _ = _arrays(torch.bfloat16, permute=None)
    got = gather_sim(xs)
    as_f32 = (got.astype(np.uint32) << 16).view(np.float32)
    f32 = [PencilArray(x.pencil, x.rank, x.data.to(torch.float32)) for x in xs]
    want = gather_sim(f32)
    assert np.array_equal(as_f32.view(np.uint32), want.view(np.uint32))


def test_gather_sim_float16_unchanged():
    xs, twins = _arrays(torch.float16)
    got = gather_sim(xs)
    assert got.dtype == np.float16
    assert np.array_equal(got.view(np.int16), gather_sim(twins))


def test_dtype_helper():
    assert numpy_dtype(torch.float16) == np.dtype(np.float16)
    assert numpy_dtype(torch.bool) == np.dtype(np.bool_)
    assert numpy_dtype(torch.bfloat16) is None
    assert bits_dtype(torch.bfloat16) == np.dtype(np.uint16)
    assert bits_dtype(torch.int8) == np.dtype(np.int8)
    t = torch.tensor([1.0, -2.5, 3.0], dtype=torch.bfloat16)
    a = to_numpy(t)
    assert a.dtype == np.uint16
    assert a.tolist() == [0x3F80, 0xC020, 0x4040]
    # non-contiguous views convert too
    m = torch.arange(12, dtype=torch.float32).to(torch.bfloat16).view(3, 4)
    assert np.array_equal(to_numpy(m.t()), to_numpy(m).T)


def test_pencilio_bfloat16_is_unsupported_element_type(tmp_path):
    topo = Topology((1, 1))
    p = Pencil(topo, DIMS, (1, 2))
    x = PencilArray(p, 0, torch.zeros(p.length_local(0),
                                      dtype=torch.bfloat16))
    path = str(tmp_path / "bf16.bin")
    f = MPIIOFile(path, "w", rank=0)
    with pytest.raises(TypeError, match="unsupported element type bfloat16"):
        f.write("u", x)
    assert f.position == 0 and "u" not in f.meta["datasets"]

    # a float16 dataset written fine is not readable into bfloat16 either
    h = PencilArray(p, 0, torch.ones(p.length_local(0), dtype=torch.float16))
    f.write("h", h)
    f.close()
    r = MPIIOFile(path, "r", rank=0)
    with pytest.raises(TypeError, match="unsupported element type bfloat16"):
        r.read("h", x)
    with pytest.raises(TypeError, match="unsupported element type bfloat16"):
        r.read_raw(x)
    back = PencilArray(p, 0, torch.zeros(p.length_local(0),
                                         dtype=torch.float16))
    r.read("h", back)
    assert torch.equal(back.data, h.data)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "int8", "uint8",
                                   "int16", "bool"])
def test_empty_with_device_is_torch_storage(dtype):
    topo = Topology((1, 1))
    p = Pencil(topo, DIMS, (1, 2))
    x = PencilArray.empty(p, 0, dtype=dtype, device="cpu")
    assert x.is_torch and x.data.dtype == getattr(torch, dtype)
    assert x.data.numel() == p.length_local(0)
    p2 = Pencil(topo, DIMS, (0, 2), permute=(1, 2, 0))
    m = ManyPencilArray([p, p2], 0, dtype=dtype, device="cpu")
    assert m.first.is_torch and m.first.data.dtype == getattr(torch, dtype)
    # without a device the default stays numpy
    assert not PencilArray.empty(p, 0, dtype="float32").is_torch
