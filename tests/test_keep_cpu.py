"""Truncated transposes, host side (no GPU): the sub-box tables of keep
plans against a brute-force count, native vs Python parity, staging and fill
coverage, the numpy mirror against the C oracle on the masked input, launch
rows, the fill's store width, and the error paths."""

from __future__ import annotations

import math
import os

import numpy as np
import pytest

from keep_util import (
    CFG_22, CFG_SLAB, CPU_CFGS, KEEP_NAMES, cfg_id, expected_keep, full_keep,
    keep_sets, pair_counts,
)
from many_util import expected_workgroups, random_parents

from pencilarrays_amd import (
    ManyPencilArray,
    MultiTransposition,
    Pencil,
    PencilArray,
    Topology,
    Transposition,
    build_plan,
    fourier_keep,
    native,
    run_transpose_sim,
    run_transpose_sim_many,
)
from pencilarrays_amd.plan import (
    buffer_nelem_many,
    copydesc_many,
    copydesc_sub,
    nsub,
    peer_message,
    stage_descs,
)

SENT = 0xAB
CASES = [(c, k) for c in CPU_CFGS for k in KEEP_NAMES]


def _case_id(v):
    return cfg_id(v) if isinstance(v, tuple) else str(v)


def _pencils(cfg):
    dims, pdims, di, pi, do, po, _ = cfg
    topo = Topology(pdims)
    return (topo, Pencil(topo, dims, di, permute=pi),
            Pencil(topo, dims, do, permute=po))


def _tup(d):
    return (d.dims, d.sstrides, d.soffset, d.dstrides, d.doffset)


# ---- sizes against the brute-force count -------------------------------

@pytest.mark.parametrize("cfg,kname", CASES, ids=_case_id)
def test_plan_sizes_equal_brute_force_count(cfg, kname):
    keep = keep_sets(cfg)[kname]
    topo, Pi, Po = _pencils(cfg)
    extra = cfg[6]
    pex = math.prod(extra or (1,))
    esz = 8
    counts = pair_counts(cfg, keep)
    nr = topo.nranks
    plans = [build_plan(Pi, Po, r, extra, keep=keep) for r in range(nr)]
    nats = [native.NativePlan(Pi, Po, r, esz, extra, keep=keep)
            for r in range(nr)]
    dropped = 0
    for r in range(nr):
        pl = plans[r]
        assert pl.r_dim is not None
        send = recv = 0
        for blk in pl.peers:
            q = blk.global_rank
            assert blk.send_nelem == counts[r][q] * pex, (r, q)
            assert blk.recv_nelem == counts[q][r] * pex, (r, q)
            if blk.peer_k == pl.my_k:
                continue
            send += blk.send_nelem
            recv += blk.recv_nelem
            for n in (1, 3):
                msg = nats[r].peer_message(n, blk.peer_k)
                assert msg == tuple(v * esz for v in
                                    peer_message(pl, n, blk.peer_k))
                assert msg[1] == n * counts[r][q] * pex * esz
                assert msg[3] == n * counts[q][r] * pex * esz
                # the sender's bytes are the receiver's
                back = nats[q].peer_message(n, pl.my_k)
                assert back[3] == msg[1] and back[1] == msg[3]
            if blk.send_nelem == 0:
                dropped += 1
                assert not blk.pack_subs
        for n in (1, 3):
            assert buffer_nelem_many(pl, n) == (n * send, n * recv)
            assert nats[r].buffer_sizes_many(n) == (n * send * esz,
                                                    n * recv * esz)
        assert nats[r].buffer_sizes() == (send * esz, recv * esz)
    if kname in ("droprank", "nothing"):
        assert dropped > 0, "this keep set should empty some message"
    if kname == "two_ranges":
        assert any(len(b.pack_subs) >= 2 or len(b.unpack_subs) >= 2
                   for p in plans for b in p.peers) or \
            any(len(p.local_subs) >= 2 for p in plans)


@pytest.mark.parametrize("cfg", CPU_CFGS, ids=cfg_id)
def test_full_keep_equals_ordinary_plan(cfg):
    """a + b = N on every dim: every table, size and launch row is the
    ordinary plan's, the two ranges of a dim merged into one sub-box."""
    keep = keep_sets(cfg)["full"]
    topo, Pi, Po = _pencils(cfg)
    extra = cfg[6]
    for aliased in (False, True):
        for r in range(topo.nranks):
            ref = build_plan(Pi, Po, r, extra, aliased=aliased)
            pl = build_plan(Pi, Po, r, extra, aliased=aliased, keep=keep)
            nref = native.NativePlan(Pi, Po, r, 8, extra, aliased=aliased)
            nk = native.NativePlan(Pi, Po, r, 8, extra, aliased=aliased,
                                   keep=keep)
            assert not pl.fills and nk.nfill() == 0
            assert (pl.send_nelem_total, pl.recv_nelem_total) == \
                (ref.send_nelem_total, ref.recv_nelem_total)
            for n in (1, 3):
                assert nk.buffer_sizes_many(n) == nref.buffer_sizes_many(n)
                for k in range(len(ref.peers)):
                    assert nk.peer_message(n, k) == nref.peer_message(n, k)
                for f in range(n):
                    for which in range(5):
                        for k in range(len(ref.peers)):
                            a = copydesc_many(ref, n, f, which, k)
                            want = 0 if a is None else 1
                            assert nsub(pl, which, k) == want
                            assert nk.nsub(which, k) == want
                            if a is not None:
                                assert _tup(copydesc_sub(
                                    pl, n, f, which, k, 0)) == _tup(a)
                                assert nk.copydesc_sub(n, f, which, k, 0) == \
                                    nref.copydesc_many(n, f, which, k)
                for stage in range(3):
                    assert nk.stage_launches(n, stage) == \
                        nref.stage_launches(n, stage)


# ---- native against Python ----------------------------------------------

def _native_cases():
    out = [(c, k, False, 1) for c, k in CASES]
    for k in ("inside", "two_ranges", "two_dims"):
        out.append((CFG_22, k, True, 1))
        out.append((CFG_22, k, False, 3))
        out.append((CFG_22, k, True, 3))
    return out


@pytest.mark.parametrize("cfg,kname,aliased,ncomp", _native_cases(),
                         ids=_case_id)
def test_native_matches_python(cfg, kname, aliased, ncomp):
    keep = keep_sets(cfg)[kname]
    topo, Pi, Po = _pencils(cfg)
    extra = cfg[6]
    ssz = 4
    esz = ssz * ncomp
    for fill in (native.FILL_ZERO, native.FILL_NONE):
        for r in range(topo.nranks):
            pl = build_plan(Pi, Po, r, extra, aliased=aliased, keep=keep,
                            fill=fill)
            npl = native.NativePlan(Pi, Po, r, ssz, extra, aliased=aliased,
                                    ncomp=ncomp, keep=keep, fill=fill)
            assert npl.plan_keep() == (pl.keep, fill)
            assert npl.buffer_sizes() == (pl.send_nelem_total * esz,
                                          pl.recv_nelem_total * esz)
            for which in range(5):
                for k in range(len(pl.peers)):
                    ns = nsub(pl, which, k)
                    assert npl.nsub(which, k) == ns, (r, which, k)
                    for n, f in ((1, 0), (3, 0), (3, 2)):
                        for s in range(ns):
                            assert npl.copydesc_sub(n, f, which, k, s) == \
                                _tup(copydesc_sub(pl, n, f, which, k, s)), \
                                (r, which, k, s, n, f)
                        assert npl.copydesc_sub(n, f, which, k, ns) is None
            assert npl.nfill() == len(pl.fills)
            if fill == native.FILL_NONE:
                assert not pl.fills
            for i, fd in enumerate(pl.fills):
                assert npl.filldesc(i) == (fd.dims, fd.dstrides, fd.doffset)


def test_same_decomposition_keep_plan():
    """R = None: local sub-boxes plus the fill, natively and in Python."""
    dims = (16, 21, 41)
    topo = Topology((2, 2))
    Pi = Pencil(topo, dims, (1, 2))
    Po = Pencil(topo, dims, (1, 2), permute=(2, 0, 1))
    keep = [(5, 2), None, (27, 0)]
    for aliased in (False, True):
        for r in range(4):
            pl = build_plan(Pi, Po, r, keep=keep, aliased=aliased)
            npl = native.NativePlan(Pi, Po, r, 8, keep=keep, aliased=aliased)
            assert pl.r_dim is None and not pl.peers
            for which in (0, 3, 4):
                assert npl.nsub(which) == nsub(pl, which)
                for s in range(nsub(pl, which)):
                    assert npl.copydesc_sub(1, 0, which, 0, s) == \
                        _tup(copydesc_sub(pl, 1, 0, which, 0, s))
            assert (nsub(pl, 0) > 0) != aliased
            assert npl.nfill() == len(pl.fills) > 0


# ---- staging and destination coverage -----------------------------------

def _touch(seen, dims, strides, offset):
    v = np.lib.stride_tricks.as_strided(
        seen[offset:], shape=dims,
        strides=tuple(s * seen.itemsize for s in strides))
    v += 1


@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("cfg,kname", CASES, ids=_case_id)
def test_sub_boxes_tile_staging_and_destination(cfg, kname, aliased):
    keep = keep_sets(cfg)[kname]
    topo, Pi, Po = _pencils(cfg)
    extra = cfg[6]
    n = 3
    for r in range(topo.nranks):
        pl = build_plan(Pi, Po, r, extra, aliased=aliased, keep=keep)
        # the sub-boxes of a peer are consecutive and tile its range
        for blk in pl.peers:
            for subs, off, cnt in ((blk.pack_subs, blk.send_offset,
                                    blk.send_nelem),
                                   (blk.unpack_subs, blk.recv_offset,
                                    blk.recv_nelem)):
                if blk.peer_k == pl.my_k:
                    assert not subs
                    continue
                o = off
                for sb in subs:
                    assert sb.offset == o and sb.nelem == sb.desc.nelem > 0
                    o += sb.nelem
                assert o == off + cnt
        ns, nr_ = buffer_nelem_many(pl, n)
        send_seen = np.zeros(ns, dtype=np.int32)
        recv_w = np.zeros(nr_, dtype=np.int32)   # staged self packs
        recv_r = np.zeros(nr_, dtype=np.int32)   # unpacks + self unpacks
        parent = np.zeros(Po.length_local(r) * math.prod(extra or (1,)),
                          dtype=np.int32)
        for f in range(n):
            one = np.zeros_like(parent)
            for which, d in stage_descs(pl, n, f, 0):
                _touch(send_seen if which == 1 else recv_w, d.dims,
                       d.dstrides, d.doffset)
            for stage in (1, 2):
                for which, d in stage_descs(pl, n, f, stage):
                    if which != 0:
                        _touch(recv_r, d.dims, d.sstrides, d.soffset)
                    _touch(one, d.dims, d.dstrides, d.doffset)
            # fill boxes and copy windows: disjoint, and together the parent
            for fd in pl.fills:
                _touch(one, fd.dims, fd.dstrides, fd.doffset)
            assert (one == 1).all(), (r, f)
        assert (send_seen == 1).all() and (recv_r == 1).all()
        tail = n * pl.peers[pl.my_k].recv_offset if aliased else nr_
        assert (recv_w[:tail] == 0).all() and (recv_w[tail:] == 1).all()


# ---- the numpy mirror against the C oracle on the masked input -----------

ELEMS = [("f64", np.float64, ()), ("c64", np.complex64, ()),
         ("3xf32", np.float32, (3,))]


def _arrays(P, parents_f, dtype, extra, elem_dims):
    return [PencilArray(P, r, parents_f[r].view(dtype).copy(), extra,
                        elem_dims) for r in range(len(parents_f))]


def _sentinel_arrays(P, exp_f, dtype, extra, elem_dims):
    return [PencilArray(P, r, np.full(len(exp_f[r]), SENT, np.uint8)
                        .view(dtype), extra, elem_dims)
            for r in range(len(exp_f))]


@pytest.mark.parametrize("elem", ELEMS, ids=lambda e: e[0])
@pytest.mark.parametrize("cfg,kname", CASES, ids=_case_id)
def test_simulation_equals_masked_oracle(cfg, kname, elem, oracle_lib_path):
    keep = keep_sets(cfg)[kname]
    _, dtype, elem_dims = elem
    topo, Pi, Po = _pencils(cfg)
    dims, pdims, di, _, _, _, extra = cfg
    esz = np.dtype(dtype).itemsize * math.prod(elem_dims or (1,))
    nr = topo.nranks
    n = 3
    parents = random_parents(dims, pdims, di, extra, esz, n, oracle_lib_path)
    for fill, zero in (("zero", True), (None, False)):
        exp = expected_keep(parents, cfg, esz, keep, oracle_lib_path,
                            fill_zero=zero, sentinel=SENT)
        # one field
        srcs = _arrays(Pi, parents[0], dtype, extra, elem_dims)
        dsts = _sentinel_arrays(Po, exp[0], dtype, extra, elem_dims)
        run_transpose_sim(dsts, srcs, keep=keep, fill=fill)
        for r in range(nr):
            assert dsts[r].data.view(np.uint8).tobytes() == \
                exp[0][r].tobytes(), (fill, r)
        # three fields, one message per peer
        srcs = [_arrays(Pi, parents[f], dtype, extra, elem_dims)
                for f in range(n)]
        dsts = [_sentinel_arrays(Po, exp[f], dtype, extra, elem_dims)
                for f in range(n)]
        run_transpose_sim_many(
            [[dsts[f][r] for f in range(n)] for r in range(nr)],
            [[srcs[f][r] for f in range(n)] for r in range(nr)],
            keep=keep, fill=fill)
        for f in range(n):
            for r in range(nr):
                assert dsts[f][r].data.view(np.uint8).tobytes() == \
                    exp[f][r].tobytes(), (fill, f, r)


def test_fourier_keep():
    assert fourier_keep((16, 21, 41), 5, real_dim=0) == \
        [(6, 0), (6, 5), (6, 5)]
    assert fourier_keep((16, 21, 41), [None, 10, 3]) == \
        [None, (11, 10), (4, 3)]
    with pytest.raises(ValueError):
        fourier_keep((16, 21, 41), 8)       # 9 + 8 > 16
    fourier_keep((16, 21, 41), [8, 10, 20], real_dim=0)


# ---- chains ---------------------------------------------------------------

def test_inplace_chain_equals_masked_source():
    """x -> y -> x in place over a ManyPencilArray pair: the result is the
    source with everything outside the keep set zeroed."""
    cfg = CFG_22
    dims, pdims = cfg[0], cfg[1]
    topo, Pi, Po = _pencils(cfg)
    keep = fourier_keep(dims, [5, 6, None], real_dim=0)
    from keep_util import parent_mask
    rng = np.random.default_rng(5)
    ms = [ManyPencilArray((Pi, Po), r) for r in range(topo.nranks)]
    orig = []
    for r, m in enumerate(ms):
        m.first.data[:] = rng.standard_normal(Pi.length_local(r))
        orig.append(m.first.data.copy())
    run_transpose_sim([m[1] for m in ms], [m[0] for m in ms], keep=keep)
    run_transpose_sim([m[0] for m in ms], [m[1] for m in ms], keep=keep)
    for r, m in enumerate(ms):
        want = np.where(parent_mask(cfg, keep, r, 0), orig[r], 0.0)
        assert m.first.data.tobytes() == want.tobytes(), r


def _gloo_worker(rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        repo = os.path.dirname(here)
        for p in (repo, os.path.join(repo, "oracle"), here):
            sys.path.insert(0, p)
        from conftest import ensure_oracle_lib
        from keep_util import ID3, expected_keep
        from many_util import random_parents
        from pencilarrays_amd import Pencil, PencilArray, Topology, \
            Transposition
        cfg = ((16, 21, 41), (2, 1), (1, 2), ID3, (0, 2), (1, 2, 0), ())
        dims, pdims, di, pi, do, po, extra = cfg
        # dim 0 cut at 8: rank 1's share of the destination is dropped
        # entirely, so rank 0 -> rank 1 is a zero-byte message
        keep = [(8, 0), (14, 3), None]
        lib = ensure_oracle_lib()
        parents = random_parents(dims, pdims, di, extra, 8, 1, lib)
        exp = expected_keep(parents, cfg, 8, keep, lib)[0]
        topo = Topology(pdims)
        Pi = Pencil(topo, dims, di, permute=pi)
        Po = Pencil(topo, dims, do, permute=po)
        src = PencilArray(Pi, rank, parents[0][rank].view(np.float64).copy())
        dst = PencilArray(Po, rank, np.full(len(exp[rank]), 0xAB, np.uint8)
                          .view(np.float64))
        t = Transposition(dst, src, keep=keep)
        t.execute()
        assert dst.data.view(np.uint8).tobytes() == exp[rank].tobytes(), rank
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_gloo_world2_keep():
    import torch.multiprocessing as mp
    mp.spawn(_gloo_worker, args=(2, 29400 + os.getpid() % 500), nprocs=2,
             join=True)


# ---- launches ------------------------------------------------------------

def test_slab_launch_rows():
    """(8,) slab, 3 f64 fields, 2/3 keep on dim 0: one grouped linear pack
    row, one grouped tile unpack row, and the local stage's tile row plus ONE
    grouped fill row; workgroups are the sums of the per-descriptor grids."""
    cfg = CFG_SLAB
    dims = cfg[0]
    topo, Pi, Po = _pencils(cfg)
    keep = [(2 * dims[0] // 3, 0), None, None]   # 10 of 16: a rank boundary
    n = 3
    tiles = (native.KERNEL_TILE, native.KERNEL_TILE_VS)
    for r in range(topo.nranks):
        pl = build_plan(Pi, Po, r, keep=keep)
        npl = native.NativePlan(Pi, Po, r, 8, keep=keep)

        def grids(stage):
            tot = 0
            for f in range(n):
                for _, d in stage_descs(pl, n, f, stage):
                    kk = native.copy_kernel_kind(d, 8, 256, 256)
                    tot += expected_workgroups(_tup(d), kk, 8)
            return tot

        npack = sum(len(b.pack_subs) for b in pl.peers)
        nunpack = sum(len(b.unpack_subs) for b in pl.peers)
        rows = npl.stage_launches(n, native.STAGE_PACK)
        if npack:
            assert [(l.kind, l.grouped, l.entries, l.workgroups)
                    for l in rows] == [(native.KERNEL_LINEAR, True,
                                        npack * n, grids(0))]
        else:
            assert rows == []
        rows = npl.stage_launches(n, native.STAGE_UNPACK)
        if nunpack:
            assert len(rows) == 1 and rows[0].kind in tiles
            assert (rows[0].grouped, rows[0].entries, rows[0].workgroups) == \
                (True, nunpack * n, grids(2))
        else:
            assert rows == []
        rows = npl.stage_launches(n, native.STAGE_LOCAL)
        want = []
        if pl.local_subs:
            assert rows[0].kind in tiles
            want.append((rows[0].kind, True, len(pl.local_subs) * n,
                         grids(1)))
        if pl.fills:
            fwg = sum(-(-fd.nelem * 8 //
                        native.fill_kernel_kind(fd, 8, 256).store_bytes
                        // 256) for fd in pl.fills)
            want.append((native.KERNEL_FILL, True, len(pl.fills) * n,
                         n * fwg))
        assert [(l.kind, l.grouped, l.entries, l.workgroups)
                for l in rows] == want
    # ranks 0..4 own kept rows only, ranks 5..7 own none: all fill
    assert build_plan(Pi, Po, 7, keep=keep).local_subs == []
    assert build_plan(Pi, Po, 7, keep=keep).fills != []


def test_fill_kernel_kind_widths():
    """f32 elements: 16-byte stores when everything allows them, and each of
    base pointer, offset, stride and run length lowers the width alone."""
    K = native.KERNEL_FILL

    def kind(dims, dstr, doff, ptr, esz=4, ncomp=1):
        return native.fill_kernel_kind((dims, dstr, doff), esz, ptr, ncomp)

    assert kind((8, 5), (1, 16), 4, 256) == (K, 16)
    assert kind((8, 5), (1, 16), 4, 256 + 8) == (K, 8)     # base pointer
    assert kind((8, 5), (1, 16), 4, 256 + 4) == (K, 4)
    assert kind((8, 5), (1, 16), 2, 256) == (K, 8)         # offset
    assert kind((8, 5), (1, 16), 1, 256) == (K, 4)
    assert kind((8, 5), (1, 18), 4, 256) == (K, 8)         # stride
    assert kind((8, 5), (1, 17), 4, 256) == (K, 4)
    assert kind((6, 5), (1, 16), 4, 256) == (K, 8)         # run length
    assert kind((5, 5), (1, 16), 4, 256) == (K, 4)
    assert kind((5, 5), (1, 16), 4, 256 + 1, esz=1) == (K, 1)
    assert kind((6, 5), (1, 16), 4, 256, esz=2) == (K, 4)
    assert kind((5, 5), (1, 16), 4, 256, esz=2) == (K, 1)
    # contiguous axes merge into one run before the width is chosen
    assert kind((3, 4), (1, 3), 0, 256) == (K, 16)
    # not contiguous along axis 0: one lane per element, the element's width
    assert kind((5, 3), (7, 70), 3, 256, esz=8) == (K, 8)
    assert kind((5, 3), (7, 70), 3, 256, esz=4, ncomp=3) == (K, 4)
    assert kind((5, 3), (8, 80), 4, 256, esz=16) == (K, 16)
    assert kind((5, 3), (7, 70), 3, 256, esz=1) == (K, 1)
    # empty window
    assert kind((0, 5), (1, 16), 0, 256) == (native.KERNEL_NONE, 0)


# ---- errors ---------------------------------------------------------------

def test_errors():
    cfg = CFG_22
    dims = cfg[0]
    topo, Pi, Po = _pencils(cfg)
    for bad in ([(17, 0), None, None], [(9, 8), None, None],
                [(-1, 0), None, None], [(3, -1), None, None],
                [(3, 0), None], [(3, 0), None, None, None]):
        with pytest.raises(ValueError):
            build_plan(Pi, Po, 0, keep=bad)
    for lo, hi in (((17, 21, 41), (0, 0, 0)), ((9, 21, 41), (8, 0, 0)),
                   ((-1, 21, 41), (0, 0, 0)), ((3, 21, 41), (-1, 0, 0))):
        with pytest.raises(RuntimeError, match="a \\+ b"):
            native.NativePlan(Pi, Po, 0, 8, keep=list(zip(lo, hi)))
    with pytest.raises(ValueError):
        native.NativePlan(Pi, Po, 0, 8, keep=[(3, 0), (4, 0)])
    with pytest.raises(RuntimeError, match="fill"):
        native.NativePlan(Pi, Po, 0, 8, keep=full_keep(dims), fill=2)
    with pytest.raises(ValueError):
        build_plan(Pi, Po, 0, keep=full_keep(dims), fill="ones")
    # keep with a wire pair
    keep = [(5, 0), None, None]
    with pytest.raises(ValueError):
        native.NativePlan(Pi, Po, 0, 8, keep=[(5, 0), (21, 0), (41, 0)],
                          wire=native.WIRE_F64_F32)
    src = PencilArray.empty(Pi, 0)
    dst = PencilArray.empty(Po, 0)
    with pytest.raises(ValueError):
        Transposition(dst, src, keep=keep, wire_dtype="float32")
    with pytest.raises(ValueError):
        MultiTransposition([dst], [src], keep=keep, wire_dtype="float32")
    with pytest.raises(ValueError):
        run_transpose_sim([dst], [src], keep=keep, wire_dtype="float32")
    # pa_plan_copydesc[_many] on a keep plan name the sub-box query
    npl = native.NativePlan(Pi, Po, 0, 8, keep=[(5, 0), (21, 0), (41, 0)])
    assert npl.copydesc(0) is None
    assert "pa_plan_copydesc_sub" in npl.lib.pa_last_error().decode()
    assert npl.copydesc_many(1, 0, 0) is None
    assert "pa_plan_copydesc_sub" in npl.lib.pa_last_error().decode()
    # and the sub-box queries refuse an ordinary plan
    ordinary = native.NativePlan(Pi, Po, 0, 8)
    assert ordinary.plan_keep() is None and ordinary.nsub(0) == 0
    assert ordinary.copydesc_sub(1, 0, 0, 0, 0) is None
    assert ordinary.nfill() == 0
