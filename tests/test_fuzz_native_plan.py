"""Property fuzz of the native (C++) plan builder against the Python mirror:
150 random configurations of ``fuzz_util.draw_cfg`` (``nd`` 2..5, up to 8
ranks, random permutations, extra dims, empty ranks), every rank, ordinary and
aliased, element sizes 1, 2, 4, 8 and 16.  Block tables, sizes, messages and
normalized descriptors must be identical; half of the configurations carry a
random keep set and compare the sub-box tables and the fills too.  Host-only."""

import os

import pytest

import fuzz_util as fu
from pencilarrays_amd import build_plan
from pencilarrays_amd.plan import (
    buffer_nelem_many, copydesc_many, copydesc_sub, nsub, peer_message,
)

native = pytest.importorskip("pencilarrays_amd.native")

if not os.path.exists(native.lib_path()):
    pytest.skip("libpencilhip.so not built", allow_module_level=True)

FIRST_INDEX = 2000   # away from the trials of the other fuzz modules
PER_FLAVOUR = 75
ESZ = [1, 2, 4, 8, 16]
TRIALS = [fu.draw_cfg(fl, FIRST_INDEX + i)
          for fl in ("plain", "keep") for i in range(PER_FLAVOUR)]


def _tup(d):
    if d is None:
        return None
    return (tuple(d.dims), tuple(d.sstrides), d.soffset, tuple(d.dstrides),
            d.doffset)


def _check_common(py, nat, esz, what):
    assert nat.r_dim == (-1 if py.r_dim is None else py.r_dim), what
    assert nat.nproc_sub == py.nproc_sub, what
    assert nat.my_k == py.my_k, what
    assert nat.buffer_sizes() == (py.send_nelem_total * esz,
                                  py.recv_nelem_total * esz), what
    for blk in py.peers:
        info = nat.block_info(blk.peer_k)
        assert info[0] == blk.peer_k and info[1] == blk.global_rank, what
        assert (info[4], info[5]) == (blk.send_nelem, blk.recv_nelem), what
        if blk.peer_k != py.my_k:
            assert (info[2], info[3]) == (blk.send_offset, blk.recv_offset), \
                what
        assert bool(info[6]) == bool(blk.pack_subs), what
        assert bool(info[7]) == bool(blk.unpack_subs), what
    for n in (1, 3):
        assert nat.buffer_sizes_many(n) == tuple(
            v * esz for v in buffer_nelem_many(py, n)), what
        for blk in py.peers:
            assert nat.peer_message(n, blk.peer_k) == tuple(
                v * esz for v in peer_message(py, n, blk.peer_k)), what


@pytest.mark.parametrize("aliased", [False, True], ids=["ordinary", "aliased"])
@pytest.mark.parametrize("t", TRIALS, ids=fu.trial_id)
def test_native_plan_matches_python(t, aliased):
    Pi, Po = fu.pencils(t)
    extra = t.cfg[6]
    esz = ESZ[t.index % len(ESZ)]
    for r in range(fu.nranks(t)):
        what = (r, aliased, esz, t)
        py = build_plan(Pi, Po, r, extra, aliased=aliased, keep=t.keep,
                        fill=t.fill)
        nat = native.NativePlan(Pi, Po, r, esz, extra, aliased=aliased,
                                keep=t.keep, fill=t.fill)
        _check_common(py, nat, esz, what)
        peers = range(max(1, len(py.peers)))
        if t.keep is None:
            assert nat.plan_keep() is None
            for which in range(5):
                for k in peers:
                    assert nat.copydesc(which, k) == \
                        _tup(copydesc_many(py, 1, 0, which, k)), \
                        (which, k) + what
                    for n, f in ((1, 0), (3, 0), (3, 2)):
                        assert nat.copydesc_many(n, f, which, k) == \
                            _tup(copydesc_many(py, n, f, which, k)), \
                            (which, k, n, f) + what
            if aliased:
                assert nat.copydesc(0) is None
            else:
                assert nat.copydesc(3) is None and nat.copydesc(4) is None
            continue
        assert nat.plan_keep() == (py.keep, t.fill), what
        for which in range(5):
            for k in peers:
                ns = nsub(py, which, k)
                assert nat.nsub(which, k) == ns, (which, k) + what
                for n, f in ((1, 0), (3, 0), (3, 2)):
                    for s in range(ns):
                        assert nat.copydesc_sub(n, f, which, k, s) == \
                            _tup(copydesc_sub(py, n, f, which, k, s)), \
                            (which, k, s, n, f) + what
                    assert nat.copydesc_sub(n, f, which, k, ns) is None
        assert nat.nfill() == len(py.fills), what
        if t.fill == native.FILL_NONE:
            assert not py.fills
        for i, fd in enumerate(py.fills):
            assert nat.filldesc(i) == (fd.dims, fd.dstrides, fd.doffset), \
                (i,) + what


def test_the_trials_cover_what_they_claim():
    assert len(TRIALS) == 150
    assert sum(fu.nranks(t) >= 2 for t in TRIALS) >= 50
    assert sum(fu.has_empty_rank(t) for t in TRIALS) >= 5
    assert {len(t.cfg[0]) for t in TRIALS} == {2, 3, 4, 5}
    assert {ESZ[t.index % len(ESZ)] for t in TRIALS} == set(ESZ)
    assert sum(t.fill == native.FILL_NONE for t in TRIALS
               if t.keep is not None) >= 10
