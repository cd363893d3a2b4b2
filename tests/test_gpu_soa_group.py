"""Grouped split / join launches (PA_PLAN_GROUP_SOA) on one MI355X.

Every case goes through ``soa_group_gpu_util.run_hop``: all ranks of a grid on
ONE GPU, device slice copies standing in for the exchange, destinations
against the C oracle per component, staging against the n-field host run, the
rows asserted through the query with the real pointers before any launch,
0xAB-filled buffers with 256-byte guards.  A flagged run must also leave,
byte for byte, what the unflagged run of the same inputs leaves."""

import math

import numpy as np
import pytest

from soa_group_util import GEN, LIN, LOCAL, PACK, TILE, UNPACK
from soa_scale_util import KINDS
from scale_util import specials

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from launch_util import max_x  # noqa: E402
from soa_group_gpu_util import (  # noqa: E402
    DEV, GUARD, JOIN, SENT, SPLIT, assert_same_bytes, dev, pencils,
    references, run_hop, sentinel,
)
from test_gpu_soa import STAGE_CFGS  # noqa: E402
from pencilarrays_amd import native  # noqa: E402
from pencilarrays_amd.plan import stage_descs  # noqa: E402

ID3 = (0, 1, 2)
DIRS = pytest.mark.parametrize("direction", [SPLIT, JOIN],
                               ids=["split", "join"])
KIND_OF = {4: "f32", 8: "f64", 16: "c128"}


# ---- the stage calls, flagged against oracle and against unflagged --------

@DIRS
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", ["f32", "f64", "c128"])
@pytest.mark.parametrize("cfg", STAGE_CFGS,
                         ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}to{c[4]}")
def test_flagged_equals_oracle_and_unflagged(cfg, kind, n, direction,
                                             oracle_lib_path):
    refs = references(cfg, kind, n, direction, oracle_lib_path)
    flagged = run_hop(cfg, kind, n, direction, oracle_lib_path, refs=refs)
    plain = run_hop(cfg, kind, n, direction, oracle_lib_path, group=False,
                    refs=refs)
    assert_same_bytes(flagged, plain)


# ---- tile edges inside ONE grouped row --------------------------------------

def _tile_shape(ssz, n, direction):
    """(ti, 16): the tile of the permuted split / join, from the query."""
    d = ((40, 3, 50), (1, 2000, 40), 0, (150, 50, 1), 0)
    k = native.copy_kernel_kind_soa(d, ssz, n, direction, 4096, [4096] * n)
    assert k.kind == TILE and k.tile_j == 16
    return k.tile_i, k.tile_j


def _tile_rows(seen):
    """a ``check`` for run_hop: collects, per rank, the grouped TILE row of
    the stage that holds the staged (join) or local (split) tile entries"""
    def check(p, py, aos, fields, send, recv, n_dir=None):
        n, direction = n_dir
        stage = LOCAL if direction == SPLIT else UNPACK
        rows = [r for r in p.stage_launches_soa(n, direction, stage, aos,
                                                fields) if r.kind == TILE]
        assert len(rows) <= 1
        if rows:
            assert rows[0].grouped
            seen.append(rows[0])
    return check


@DIRS
@pytest.mark.parametrize("P", [2, 3])
def test_ragged_tiles_and_different_block_counts_in_one_row(P, direction,
                                                            oracle_lib_path):
    """A permuted slab over P ranks, f64 x 3.  Along both tile axes every
    entry has two tiles or more; with P = 3 the shares are 2T, 2T, 2T + 1, so
    the entries of one grouped row have different tile and block counts and
    the last tile of some is ragged; with P = 2 every share is 2T + 3."""
    n, kind, ssz = 3, "f64", 8
    ti, tj = _tile_shape(ssz, n, direction)
    if P == 2:
        dims = (2 * (2 * ti + 3), 2 * (2 * tj + 5), 3)
    else:
        dims = (3 * 2 * ti + 1, 3 * 2 * tj + 1, 3)
    cfg = (dims, (P,), (1,), ID3, (0,), (1, 0, 2), ())
    seen = []
    chk = _tile_rows(seen)
    refs = references(cfg, kind, n, direction, oracle_lib_path)
    flagged = run_hop(cfg, kind, n, direction, oracle_lib_path, refs=refs,
                      check=lambda *a: chk(*a, n_dir=(n, direction)))
    plain = run_hop(cfg, kind, n, direction, oracle_lib_path, group=False,
                    refs=refs)
    assert_same_bytes(flagged, plain)
    assert len(seen) == P
    # a join's unpack row holds the P - 1 peer blocks, a split's local one
    assert all(r.entries == (1 if direction == SPLIT else P - 1)
               for r in seen)
    if P == 3:   # the ranks' rows differ: shares of 2T and of 2T + 1
        assert len({r.workgroups for r in seen}) > 1


def _edge_cases():
    out = []
    for kind, ns, ks in (("f64", (2, 3, 4), (0, 1, 2)),
                         ("f32", (2, 3, 4), (1, 2)),
                         ("c128", (2, 3, 4), (1, 2))):
        for n in ns:
            for a in ks:
                for b in ks:
                    out.append((kind, n, a, b))
    return out


@DIRS
@pytest.mark.parametrize("kind,n,a,b", _edge_cases())
def test_entry_extents_at_the_tile_edges(kind, n, a, b, direction,
                                         oracle_lib_path):
    """Every entry of the grouped TILE row has extents (e0, e1) out of
    {1, T - 1, T + 1} on the two tile axes: a permuted slab over 2 ranks
    whose shares are e0 and e1."""
    ssz = KINDS[kind][1]
    T = _tile_shape(ssz, n, direction)
    e0, e1 = [(1, t - 1, t + 1)[i] for t, i in zip(T, (a, b))]
    cfg = ((2 * e0, 2 * e1, 3), (2,), (1,), ID3, (0,), (1, 0, 2), ())
    seen = []

    def check(p, py, aos, fields, send, recv):
        for stage in (1, 2):     # the local copy and the unpacks
            for which, d in stage_descs(py, n, 0, stage):
                seen.append(math.prod(d.dims))
    refs = references(cfg, kind, n, direction, oracle_lib_path)
    flagged = run_hop(cfg, kind, n, direction, oracle_lib_path, refs=refs,
                      check=check)
    plain = run_hop(cfg, kind, n, direction, oracle_lib_path, group=False,
                    refs=refs)
    assert_same_bytes(flagged, plain)
    # both ranks' local block and peer block: e0 x e1 x 3 elements each
    assert seen == [e0 * e1 * 3] * 4, seen


# ---- mixed rows --------------------------------------------------------------

@DIRS
def test_two_linear_rows_of_different_v_in_one_stage(direction,
                                                     oracle_lib_path):
    """x = 10 over 3 ranks is 3 + 3 + 4: blocks of 4 move two f32 an access,
    blocks of 3 one, so one stage call launches a row of each."""
    n, kind = 3, "f32"
    cfg = ((10, 12, 5), (3,), (1,), ID3, (0,), ID3, ())
    if direction == JOIN:   # the mirror hop: x-slabs back to y-slabs
        cfg = ((10, 12, 5), (3,), (0,), ID3, (1,), ID3, ())
    two = []

    def check(p, py, aos, fields, send, recv):
        stage = PACK if direction == SPLIT else UNPACK
        rows = p.stage_launches_soa(n, direction, stage, aos, fields)
        assert all(r.kind == LIN and r.grouped for r in rows)
        two.append(len(rows))
    refs = references(cfg, kind, n, direction, oracle_lib_path)
    flagged = run_hop(cfg, kind, n, direction, oracle_lib_path, refs=refs,
                      check=check)
    plain = run_hop(cfg, kind, n, direction, oracle_lib_path, group=False,
                    refs=refs)
    assert_same_bytes(flagged, plain)
    assert max(two) == 2, two


@DIRS
def test_generic_rows_beside_grouped_rows(direction, oracle_lib_path):
    """x = 4 over 3 ranks is 1 + 1 + 2: a block one plane thick has no
    contiguous axis on the array side and stays a SOA_GENERIC row of its own
    next to the grouped row of the same stage call; and n = 5, where every
    row is generic, through the same tables."""
    cfg = ((4, 12, 5), (3,), (1,), ID3, (0,), ID3, ())
    if direction == JOIN:   # the mirror hop: x-slabs back to y-slabs
        cfg = ((4, 12, 5), (3,), (0,), ID3, (1,), ID3, ())
    mixed = []

    def check(p, py, aos, fields, send, recv):
        for stage in ((PACK, LOCAL) if direction == SPLIT
                      else (LOCAL, UNPACK)):
            rows = p.stage_launches_soa(2, direction, stage, aos, fields)
            kinds = {r.kind for r in rows}
            assert all(r.grouped == (r.kind != GEN) for r in rows)
            mixed.append(GEN in kinds and len(kinds) > 1)
    refs = references(cfg, "f32", 2, direction, oracle_lib_path)
    flagged = run_hop(cfg, "f32", 2, direction, oracle_lib_path, refs=refs,
                      check=check)
    plain = run_hop(cfg, "f32", 2, direction, oracle_lib_path, group=False,
                    refs=refs)
    assert_same_bytes(flagged, plain)
    assert any(mixed), "no stage had a generic row beside a grouped one"
    refs = references(STAGE_CFGS[2], "f64", 5, direction, oracle_lib_path)
    assert_same_bytes(
        run_hop(STAGE_CFGS[2], "f64", 5, direction, oracle_lib_path,
                refs=refs),
        run_hop(STAGE_CFGS[2], "f64", 5, direction, oracle_lib_path,
                group=False, refs=refs))


# ---- scaled calls on a flagged plan ----------------------------------------

@DIRS
@pytest.mark.parametrize("kind", ["f32", "f64", "c64", "c128"])
def test_scaled_calls_on_a_flagged_plan(kind, direction, oracle_lib_path):
    """The four (S, R) pairs, -2 and 1/3, permuted and not."""
    for cfg, alpha in ((STAGE_CFGS[0], -2.0), (STAGE_CFGS[2], 1.0 / 3.0)):
        refs = references(cfg, kind, 3, direction, oracle_lib_path,
                          alpha=alpha)
        flagged = run_hop(cfg, kind, 3, direction, oracle_lib_path,
                          alpha=alpha, refs=refs)
        plain = run_hop(cfg, kind, 3, direction, oracle_lib_path,
                        alpha=alpha, group=False, refs=refs)
        assert_same_bytes(flagged, plain)


def _slab2(kind, n, group=True):
    """rank 0 of a permuted slab over 2 ranks with its staging, and rank 1's
    plan for the message ranges"""
    cfg = ((24, 20, 6), (2,), (1,), ID3, (0,), (1, 0, 2), ())
    Pi, Po, nr, extra = pencils(cfg)
    ssz = KINDS[kind][1]
    plans = [native.NativePlan(Pi, Po, r, ssz, extra, group_soa=group)
             for r in range(nr)]
    return cfg, Pi, Po, plans


@pytest.mark.parametrize("kind", ["f32", "f64", "c64", "c128"])
def test_specials_through_pack_slice_copy_unpack(kind):
    """Every special value of the real type rides rank 0's scaled split pack
    into staging, a device slice copy to rank 1's recv buffer, and rank 1's
    ordinary unpack; and back through a scaled join's unpack.  Staging holds
    the reference-scaled scalars for a split, the plain ones for a join."""
    dt, ssz, R, code = KINDS[kind]
    n, alpha = 2, 0.5
    cfg, Pi, Po, plans = _slab2(kind, n)
    nreal = Pi.length_local(0) * n * (ssz // R.itemsize)
    sp = specials(R)
    vals = np.resize(sp, nreal).astype(R)
    raw = vals.view(np.uint8)
    a_t = dev(raw)
    sizes = [p.buffer_sizes_many(n) for p in plans]
    sends = [sentinel(s) for s, _ in sizes]
    recvs = [sentinel(r) for _, r in sizes]
    for r, p in enumerate(plans):
        p.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    rows = plans[0].stage_launches_soa(n, SPLIT, PACK, a_t.data_ptr())
    assert [(r.kind, r.grouped, r.entries) for r in rows] == [(LIN, True, 1)]
    plans[0].pack_split_scaled(n, code, alpha, a_t.data_ptr(), stream)
    so, sn, _, _ = plans[0].peer_message(n, 1)
    _, _, ro, rn = plans[1].peer_message(n, 0)
    assert sn == rn and sn > 0
    recvs[1][ro:ro + rn] = sends[0][so:so + sn]
    # the staged scalars: a permutation of the scaled source's, so compare
    # as sorted bit patterns, NaNs counted
    U = {4: np.uint32, 8: np.uint64}[R.itemsize]
    got = recvs[1][ro:ro + rn].cpu().numpy().view(R)
    # rank 0 sends x in rank 1's share: half of its scalars
    src = vals.reshape(-1, 24, n * (ssz // R.itemsize))[:, 12:, :]
    with np.errstate(all="ignore"):
        want = (src * R.type(alpha)).reshape(-1)
    assert np.isnan(got).sum() == np.isnan(want).sum() > 0
    g, w = got[~np.isnan(got)], want[~np.isnan(want)]
    assert np.array_equal(np.sort(g.view(U)), np.sort(w.view(U)))
    # rank 1's join unpack of the same message, scaled again: 0.25 x source
    out = sentinel(Po.length_local(1) * n * ssz)
    plans[1].unpack_join_scaled(n, code, alpha, out.data_ptr(), stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[-GUARD:] == SENT).all()
    body = o[:-GUARD].view(R)
    written = body[body.view(U) != U(int.from_bytes(bytes([SENT]) *
                                                    R.itemsize, "little"))]
    with np.errstate(all="ignore"):
        want2 = (want * R.type(alpha)).reshape(-1)
    assert np.isnan(written).sum() == np.isnan(want2).sum()
    assert np.array_equal(np.sort(written[~np.isnan(written)].view(U)),
                          np.sort(want2[~np.isnan(want2)].view(U)))
    for p in plans:
        p.set_buffers(0, 0)


@DIRS
def test_alpha_is_not_part_of_a_table(direction, oracle_lib_path):
    """A plain call, scaled calls with two alphas and a plain call again on
    the same arrays: the tables of the first call serve them all, and
    alpha == 1.0 leaves the plain call's bytes, NaN payloads included."""
    kind, n = "f64", 3
    dt, ssz, R, code = KINDS[kind]
    cfg, Pi, Po, plans = _slab2(kind, n)
    p = plans[0]
    rng = np.random.default_rng(7)
    split = direction == SPLIT
    nel = (Pi if split else Po).length_local(0) * n
    a_host = rng.integers(0, 256, nel * ssz, dtype=np.uint8)  # NaNs included
    a_t = dev(a_host) if split else sentinel(nel * ssz)
    fl = (Po if split else Pi).length_local(0) * ssz
    f_t = [sentinel(fl) if split else
           dev(rng.integers(0, 256, fl, dtype=np.uint8)) for _ in range(n)]
    fp = [t.data_ptr() for t in f_t]
    sb, rb = p.buffer_sizes_many(n)
    send, recv = sentinel(sb), sentinel(rb)
    recv[:rb] = dev(rng.integers(0, 256, rb, dtype=np.uint8))
    p.set_buffers(send.data_ptr(), recv.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream

    def run(alpha):
        if split:
            if alpha is None:
                p.pack_split(n, a_t.data_ptr(), stream)
                p.local_split(a_t.data_ptr(), fp, stream)
            else:
                p.pack_split_scaled(n, code, alpha, a_t.data_ptr(), stream)
                p.local_split_scaled(code, alpha, a_t.data_ptr(), fp, stream)
        elif alpha is None:
            p.local_join(fp, a_t.data_ptr(), stream)
            p.unpack_join(n, a_t.data_ptr(), stream)
        else:
            p.local_join_scaled(code, alpha, fp, a_t.data_ptr(), stream)
            p.unpack_join_scaled(n, code, alpha, a_t.data_ptr(), stream)
        torch.cuda.synchronize()
        outs = ([send] + f_t) if split else [a_t]
        return [t.cpu().numpy().copy() for t in outs]

    plain = run(None)
    builds = p.stage_table_builds()
    assert builds == 2 and p.stage_table_count() == 2
    a0 = torch.cuda.memory_allocated()
    half = run(0.5)
    third = run(1.0 / 3.0)
    one = run(1.0)
    again = run(None)
    assert p.stage_table_builds() == builds and p.stage_table_count() == 2
    assert torch.cuda.memory_allocated() == a0
    for x, y in zip(plain, one):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(plain, again):
        assert x.tobytes() == y.tobytes()
    assert any(x.tobytes() != y.tobytes() for x, y in zip(plain, half))
    assert any(x.tobytes() != y.tobytes() for x, y in zip(half, third))
    # set_buffers drops the tables like the others
    p.set_buffers(send.data_ptr(), recv.data_ptr())
    assert p.stage_table_count() == 0
    p.set_buffers(0, 0)


# ---- launch geometry --------------------------------------------------------

def test_join_tile_row_past_the_grid_split():
    """Rank 0 of a permuted slab over 4 ranks with shares of 2 x 2 and z = B:
    its join unpack is ONE grouped SOA_TILE row of three (2, 2, B) entries,
    one workgroup per 2 x 2 batch.  3 B passes the gridDim.x limit of a
    256-wide workgroup, so the second grid row does real work, and the row
    boundary falls inside the third entry.  f64 x 2.  The reference is torch
    indexing on the device: the buffers are a GiB each."""
    n, ssz = 2, 8
    B = max_x(256) // 3 + 3
    dims = (8, 8, B)
    topo_cfg = (dims, (4,), (1,), ID3, (0,), (1, 0, 2), ())
    Pi, Po, nr, extra = pencils(topo_cfg)
    p = native.NativePlan(Pi, Po, 0, ssz, extra, group_soa=True)
    flat = native.NativePlan(Pi, Po, 0, ssz, extra)
    sb, rb = p.buffer_sizes_many(n)
    assert rb == 3 * 4 * B * n * ssz
    send = sentinel(0)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    recv = torch.randint(-2 ** 62, 2 ** 62, (rb // 8 + GUARD // 8,),
                         dtype=torch.int64, device=DEV, generator=g)
    out = torch.full((Po.length_local(0) * n + GUARD // 8,), -1,
                     dtype=torch.int64, device=DEV)
    p.set_buffers(send.data_ptr(), recv.data_ptr())
    flat.set_buffers(send.data_ptr(), recv.data_ptr())
    rows = p.stage_launches_soa(n, JOIN, UNPACK, out.data_ptr())
    un = flat.stage_launches_soa(n, JOIN, UNPACK, out.data_ptr())
    assert [(u.kind, u.grouped, u.workgroups) for u in un] == \
        [(TILE, False, B)] * 3
    assert [tuple(r) for r in rows] == [(TILE, True, 3, 3 * B)]
    assert 2 * B < max_x(256) < 3 * B     # the boundary: inside entry 3
    p.unpack_join(n, out.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    # rank 0's destination: x in [0, 2), memory order (y, x, z) with y
    # fastest, n components fastest of all; y in [0, 2) is the local block
    # (not written here).  The block of peer k holds, per component slot,
    # (x, y_k, z) column-major in Pi's memory order: x fastest.
    o = out[:Po.length_local(0) * n].view(B, 2, 8, n)      # z, x, y, c
    cnt = 4 * B
    for i, k in enumerate((1, 2, 3)):
        blk = recv[i * cnt * n:(i + 1) * cnt * n].view(n, B, 2, 2)  # c z y x
        want = blk.permute(1, 3, 2, 0)                     # z, x, y, c
        assert torch.equal(o[:, :, 2 * k:2 * k + 2, :], want), k
    assert bool((o[:, :, 0:2, :] == -1).all())
    assert bool((out[Po.length_local(0) * n:] == -1).all())
    p.set_buffers(0, 0)
    flat.set_buffers(0, 0)
    del recv, out
    torch.cuda.empty_cache()
