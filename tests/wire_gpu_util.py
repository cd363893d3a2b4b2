"""Device-side helpers of the reduced-precision wire tests: a
pa_device_copy_wire runner that asserts the selection first and compares the
WHOLE sentinel-filled destination with a host reference, and the stage API
run as a multi-rank transpose on one GPU."""

from __future__ import annotations

import numpy as np
import torch

from pencilarrays_amd import Pencil, Topology, build_plan, native
from wire_util import (
    ELEM_KINDS, NARROW, PAIRS, ROUND, WIDEN, assert_same, carrier,
    expected_rounded, kind_parents, ref_narrow, ref_round, ref_widen,
    seeded_values,
)

GUARD = 256   # guard bytes behind every destination and staging buffer
SENT = 0xAB
CVT = {native.KERNEL_CVT_LINEAR, native.KERNEL_CVT_TILE,
       native.KERNEL_CVT_GENERIC}


def side_types(pair, op):
    """(src, dst) numpy scalar types of a converting copy."""
    stored, w = np.dtype(PAIRS[pair][0]), carrier(pair)
    return (w if op == WIDEN else stored), (w if op == NARROW else stored)


def ref_conv(pair, op):
    return {NARROW: ref_narrow, WIDEN: ref_widen, ROUND: ref_round}[op], pair


def source_values(n, pair, op, seed):
    """``n`` source scalars of the op's source type, special values mixed in
    (for WIDEN: their wire images, so inf, subnormals and a NaN go in)."""
    x = seeded_values(n, pair, seed)
    return ref_narrow(x, pair) if op == WIDEN else x


def extent(dims, strides, offset, nc=1):
    """Scalars a buffer needs to hold every index the descriptor touches."""
    if 0 in dims:
        return 0
    return (offset + 1 + sum((d - 1) * s for d, s in zip(dims, strides))) * nc


def ref_copy(desc, src, dst, nc, pair, op):
    """The descriptor on the host, converting with the references."""
    dims, sstr, soff, dstr, doff = desc
    if 0 in dims:
        return
    si, di = src.itemsize, dst.itemsize
    ast = np.lib.stride_tricks.as_strided
    shape = tuple(dims) + (nc,)
    sv = ast(src[soff * nc:], shape=shape,
             strides=tuple(s * nc * si for s in sstr) + (si,))
    dv = ast(dst[doff * nc:], shape=shape,
             strides=tuple(s * nc * di for s in dstr) + (di,))
    fn, p = ref_conv(pair, op)
    dv[...] = fn(np.ascontiguousarray(sv).reshape(-1), p).reshape(shape)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()) \
        .to("cuda:0")


def sentinel(nbytes):
    return torch.full((nbytes + GUARD,), SENT, dtype=torch.uint8,
                      device="cuda:0")


def run_copy(desc, pair, op, nc, seed, want_kind, want_vec=None,
             src_lead=0, dst_lead=0, slack=4):
    """Run ``desc`` (element units) through pa_device_copy_wire.  Buffers are
    just large enough plus ``slack`` scalars and a guard; ``*_lead`` moves
    that base pointer so many SCALARS into its allocation.  The selection is
    asserted with the real pointers before the copy runs; the whole
    destination (lead, data, slack, guard) is compared.  Returns the
    selection."""
    dims, sstr, soff, dstr, doff = desc
    st, dt = side_types(pair, op)
    code = PAIRS[pair][2]
    src = source_values(extent(dims, sstr, soff, nc) + slack, pair, op, seed)
    assert src.dtype == st
    dst_n = extent(dims, dstr, doff, nc) + slack
    exp = np.empty(dst_n, dtype=dt)
    exp.view(np.uint8)[:] = SENT
    ref_copy(desc, src, exp, nc, pair, op)

    s_all = torch.cat([torch.full((src_lead * st.itemsize,), 0x5C,
                                  dtype=torch.uint8, device="cuda:0"),
                       dev(src)])
    s_t = s_all[src_lead * st.itemsize:]
    d_all = sentinel(dst_lead * dt.itemsize + dst_n * dt.itemsize)
    d_t = d_all[dst_lead * dt.itemsize:]
    k = native.copy_kernel_kind_wire(desc, code, op, nc, s_t.data_ptr(),
                                     d_t.data_ptr())
    what = f"{pair} op={op} nc={nc} {desc} lead=({src_lead},{dst_lead}) {k}"
    assert k.kind == want_kind, what
    if want_vec is not None:
        assert k.vec == want_vec, what
    native.device_copy_wire(desc, code, op, nc, s_t.data_ptr(),
                            d_t.data_ptr())
    torch.cuda.synchronize()
    got = d_all.cpu().numpy()
    lead_b, nb = dst_lead * dt.itemsize, dst_n * dt.itemsize
    assert (got[:lead_b] == SENT).all(), what + " lead"
    assert (got[lead_b + nb:] == SENT).all(), what + " guard"
    assert_same(got[lead_b:lead_b + nb].view(dt), exp, what)
    return k


def transpose_desc(n0, nta, nb, s_pitch, soff, d_pitch, doff, ta_pos=1):
    """src unit-stride along axis 0 with row pitch ``s_pitch``, dst
    unit-stride along the ta axis with row pitch ``d_pitch``, batch ``nb``.
    ``ta_pos`` = where ta lands in the normalized (src-stride-sorted)
    descriptor: 1 = right after axis 0, 2 = behind the batch axis."""
    if ta_pos == 1:
        return ((n0, nta, nb), (1, s_pitch, s_pitch * nta), soff,
                (d_pitch, 1, d_pitch * n0), doff)
    return ((n0, nb, nta), (1, s_pitch, s_pitch * nb), soff,
            (d_pitch, d_pitch * n0, 1), doff)


def _stage_kinds(p, py, n, code, nc, sp, dp, send, recv):
    """The selection of every descriptor of the three stages through the
    query, in the order the stage calls launch them."""
    def q(f, which, k, op, s, d):
        desc = p.copydesc_many(n, f, which, k)
        kk = native.copy_kernel_kind_wire(desc, code, op, nc, s, d)
        return [] if kk.kind == native.KERNEL_NONE else [kk.kind]

    pack, local, unpack = [], [], []
    for f in range(n):
        for b in py.peers:
            if b.pack is not None:
                pack += q(f, 1, b.peer_k, NARROW, sp[f], send)
        if py.self_pack is not None:
            pack += q(f, 3, 0, NARROW, sp[f], recv)
        if py.local is not None:
            local += q(f, 0, 0, ROUND, sp[f], dp[f])
        if py.self_unpack is not None:
            local += q(f, 4, 0, WIDEN, recv, dp[f])
        for b in py.peers:
            if b.unpack is not None:
                unpack += q(f, 2, b.peer_k, WIDEN, recv, dp[f])
    return pack, local, unpack


def run_stage_sim(cfg, kind, n, oracle_lib_path, aliased=False):
    """All ranks of ``cfg`` on one GPU through the stage API of wire plans:
    pack_many -> one device slice copy per peer pair at the peer_message
    ranges -> local_many -> unpack_many.  Asserts the launches against the
    query, destinations == the C oracle on the reference-rounded input, and
    every guard."""
    dims, pdims, di, pi, do, po, extra = cfg
    dtype, elem, pair, nc = ELEM_KINDS[kind]
    stored = np.dtype(PAIRS[pair][0]).itemsize
    code = PAIRS[pair][2]
    topo = Topology(pdims)
    Pi = Pencil(topo, dims, di, permute=pi)
    Po = Pencil(topo, dims, do, permute=po)
    nr = topo.nranks
    parents = kind_parents(kind, dims, pdims, di, extra, n, oracle_lib_path)
    exp = expected_rounded(kind, parents, cfg, oracle_lib_path)

    pyplans = [build_plan(Pi, Po, r, extra, aliased=aliased)
               for r in range(nr)]
    plans = [native.NativePlan(Pi, Po, r, stored, extra, aliased=aliased,
                               ncomp=nc, wire=code) for r in range(nr)]
    srcs = [[dev(parents[f][r]) if parents[f][r].size else sentinel(0)
             for f in range(n)] for r in range(nr)]
    dsts = [[sentinel(exp[f][r].nbytes) for f in range(n)]
            for r in range(nr)]
    sizes = [p.buffer_sizes_many(n) for p in plans]
    sends = [sentinel(s) for s, _ in sizes]
    recvs = [sentinel(rb) for _, rb in sizes]
    for r, p in enumerate(plans):
        p.set_buffers(sends[r].data_ptr(), recvs[r].data_ptr())
    sp = [[t.data_ptr() for t in srcs[r]] for r in range(nr)]
    dp = [[t.data_ptr() for t in dsts[r]] for r in range(nr)]
    for r, p in enumerate(plans):
        want = _stage_kinds(p, pyplans[r], n, code, nc, sp[r], dp[r],
                            sends[r].data_ptr(), recvs[r].data_ptr())
        for stage, w in zip((native.STAGE_PACK, native.STAGE_LOCAL,
                             native.STAGE_UNPACK), want):
            rows = p.stage_launches(n, stage, sp[r], dp[r])
            assert [l.kind for l in rows] == w, (r, stage, rows, w)
            assert all(l.kind in CVT and not l.grouped for l in rows)

    stream = torch.cuda.current_stream().cuda_stream
    for r, p in enumerate(plans):
        p.pack_many(sp[r], stream)
    for r, p in enumerate(plans):
        for blk in pyplans[r].peers:
            if blk.peer_k == pyplans[r].my_k:
                continue
            so, sn, _, _ = p.peer_message(n, blk.peer_k)
            _, _, ro, rn = plans[blk.global_rank].peer_message(
                n, pyplans[r].my_k)
            assert sn == rn
            if sn:
                recvs[blk.global_rank][ro:ro + rn] = sends[r][so:so + sn]
    for r, p in enumerate(plans):
        p.local_many(sp[r], dp[r], stream)
        p.unpack_many(dp[r], stream)
    torch.cuda.synchronize()

    for r in range(nr):
        for f in range(n):
            nb = exp[f][r].nbytes
            got = dsts[r][f].cpu().numpy()
            assert_same(got[:nb].view(dtype), exp[f][r],
                        f"rank {r} field {f}")
            assert (got[nb:] == SENT).all(), f"rank {r} field {f} guard"
        for t, nbytes, name in ((sends[r], sizes[r][0], "send"),
                                (recvs[r], sizes[r][1], "recv")):
            assert bool((t[nbytes:] == SENT).all().item()), \
                f"rank {r} {name} guard"
    for p in plans:  # tables die with the staging they point into
        p.set_buffers(0, 0)
