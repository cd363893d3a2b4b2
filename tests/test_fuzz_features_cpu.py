"""Property fuzz of the plan flavours on the CPU, as an independent line next
to the device fuzz (test_gpu_fuzz_multirank.py):

- the numpy mirror (``run_transpose_sim_many`` with ``keep``, ``scale``,
  ``wire_dtype`` and ``n > 1``, ``run_transpose_sim_split`` / ``_join``) on
  random multi-rank trials of ``fuzz_util.draw_cfg`` against the DIRECT-SPEC
  oracle (``oracle.transpose_oracle``: assemble the global array, slice it)
  with the feature applied in numpy, in place too where the flavour allows.
  The device fuzz leans on the C oracle; its expected destinations
  (``fuzz_util.host_case``) must equal this line bit for bit as well;
- a self-test of the comparison the device fuzz uses: it must fail when the
  buffers it is given are the expected output of a slightly wrong
  configuration."""

import numpy as np
import pytest

import fuzz_util as fu
import keep_util
import oracle as orc
import scale_util
import wire_util
from pencilarrays_amd import (
    PencilArray, native, run_transpose_sim_join, run_transpose_sim_many,
    run_transpose_sim_split,
)

SENT = fu.SENT
PER_FLAVOUR = 10
FIRST_INDEX = 1000   # away from the device fuzz's trials


def multirank_trials(flavour):
    """The first PER_FLAVOUR trials from FIRST_INDEX on with two or more
    ranks (and, for the plain flavour, two or more fields)."""
    out, i = [], FIRST_INDEX
    while len(out) < PER_FLAVOUR:
        t = fu.draw_cfg(flavour, i)
        i += 1
        if fu.nranks(t) >= 2 and (flavour != "plain" or t.n > 1):
            out.append(t)
    return out


CPU_FLAVOURS = ("plain", "keep", "wire", "scale", "split", "join")
TRIALS = [t for fl in CPU_FLAVOURS for t in multirank_trials(fl)]


def _void(a, esz):
    """Bytes as opaque elements of ``esz`` bytes, which numpy moves whole."""
    return a.view(np.dtype((np.void, esz)))


def _direct(parents_u8, cfg, esz, keep=None, fill_zero=True):
    """Per-rank destination bytes by the direct-spec oracle on opaque
    elements; with ``keep`` the global array is masked in numpy first and the
    complement is zero or the sentinel."""
    dims, pdims, di, pi, do, po, extra = cfg
    parents = [_void(p, esz) for p in parents_u8]
    nr = len(parents)
    if keep is None:
        exp = orc.transpose_oracle(parents, dims, pdims, di, pi, do, po,
                                   extra)
        return [e.view(np.uint8).reshape(-1) for e in exp]
    g = orc.global_from_parents(parents, dims, pdims, di, pi, extra)
    K = keep_util.keep_mask(dims, keep)
    K = np.broadcast_to(K.reshape(K.shape + (1,) * len(extra)), g.shape)
    g = g.copy()
    bg = g.view(np.uint8).reshape(g.shape + (esz,))
    bg[~K] = 0 if fill_zero else SENT
    return [orc.parent_from_global(g, dims, pdims, do, po, r, extra)
            .view(np.uint8).reshape(-1) for r in range(nr)]


def direct_expected(t, case):
    """``exp[r][j]`` bytes for a trial, independent of the C oracle."""
    cfg, n, nr = t.cfg, t.n, fu.nranks(t)
    zero = t.fill == native.FILL_ZERO
    if t.flavour in ("plain", "keep"):
        esz = t.elem[0] * t.elem[1]
        per_f = [_direct([case.srcs[r][f] for r in range(nr)], cfg, esz,
                         t.keep, zero) for f in range(n)]
    elif t.flavour == "wire":
        pair, nc = t.elem
        stored = np.dtype(wire_util.PAIRS[pair][0])
        per_f = [_direct([fu._u8(wire_util.ref_round(
            case.srcs[r][f].view(stored), pair)) for r in range(nr)], cfg,
            stored.itemsize * nc) for f in range(n)]
    elif t.flavour == "scale":
        dtype, _, S, _, nscal = scale_util.KINDS[t.elem]
        per_f = [_direct([fu._u8(scale_util.ref_scale(
            case.srcs[r][f].view(dtype), t.alpha)) for r in range(nr)], cfg,
            np.dtype(S).itemsize * nscal, t.keep, zero) for f in range(n)]
    elif t.flavour == "split":
        ssz = t.elem
        per_f = [_direct([np.ascontiguousarray(
            case.srcs[r][0].reshape(-1, n, ssz)[:, c]).reshape(-1)
            for r in range(nr)], cfg, ssz) for c in range(n)]
    else:
        ssz = t.elem
        per_c = [_direct([case.srcs[r][c] for r in range(nr)], cfg, ssz)
                 for c in range(n)]
        return [[np.ascontiguousarray(np.stack(
            [per_c[c][r].reshape(-1, ssz) for c in range(n)], axis=1))
            .reshape(-1)] for r in range(nr)]
    return [[per_f[f][r] for f in range(len(per_f))] for r in range(nr)]


def _mirror(t, case, inplace):
    """The numpy mirror on the trial's inputs; returns ``got[r][j]`` as the
    device driver reads destinations back (lead, data, guard)."""
    Pi, Po = fu.pencils(t)
    extra, n, nr = t.cfg[6], t.n, fu.nranks(t)
    tname, elem_dims = fu.array_type(t)
    dt = np.dtype(tname)
    s_ed = (n,) if t.flavour == "split" else elem_dims
    d_ed = (n,) if t.flavour == "join" else elem_dims
    srcs, dsts, raws = [], [], []
    for r in range(nr):
        s_row, d_row, raw_row = [], [], []
        for j, a in enumerate(case.srcs[r]):
            e = case.exp[r][j] if inplace else None
            buf = np.full(max(a.size, e.size) if inplace else a.size, SENT,
                          dtype=np.uint8)
            buf[:a.size] = a
            s_row.append(PencilArray(Pi, r, buf[:a.size].view(dt), extra,
                                     s_ed))
            if inplace:
                raw_row.append(buf)
        for j, e in enumerate(case.exp[r]):
            buf = raw_row[j] if inplace else np.full(e.size, SENT, np.uint8)
            if not inplace:
                raw_row.append(buf)
            d_row.append(PencilArray(Po, r, buf[:e.size].view(dt), extra,
                                     d_ed))
        srcs.append(s_row)
        dsts.append(d_row)
        raws.append(raw_row)
    if t.flavour == "split":
        run_transpose_sim_split(dsts, [row[0] for row in srcs])
    elif t.flavour == "join":
        run_transpose_sim_join([row[0] for row in dsts], srcs)
    else:
        kw = {}
        if t.keep is not None:
            kw.update(keep=list(t.keep),
                      fill="zero" if t.fill == native.FILL_ZERO else None)
        if t.flavour == "scale":
            kw.update(scale=t.alpha)
        if t.flavour == "wire":
            kw.update(wire_dtype=wire_util.PAIRS[t.elem[0]][1])
        run_transpose_sim_many(dsts, srcs, **kw)
    return [[raws[r][j][:e.size] for j, e in enumerate(case.exp[r])]
            for r in range(nr)]


@pytest.mark.parametrize("t", TRIALS, ids=fu.trial_id)
def test_numpy_mirror_vs_direct_spec_oracle(t, oracle_lib_path):
    t = t._replace(lead=None, aliased=False)   # host arrays: no pointers
    case = fu.host_case(t, oracle_lib_path)
    exp = direct_expected(t, case)
    direct = case._replace(exp=exp)
    # the device fuzz's reference (C oracle) against the direct-spec line
    fu.compare_dst(t, direct, fu.as_got(t, case.exp))
    fu.compare_dst(t, direct, fu.as_got(t, _mirror(t, case, False)))
    # in place: one buffer per field and rank holds both sides.  What a
    # fill of none leaves behind is then the source's own bytes, so only
    # zero-filled keeps run in place
    if t.flavour in fu.CAN_ALIAS and not (
            t.keep is not None and t.fill == native.FILL_NONE):
        fu.compare_dst(t, direct, fu.as_got(t, _mirror(t, case, True)))


# ---- the comparison must tell a slightly wrong configuration apart --------

CFG = ((12, 7, 10), (2, 2), (1, 2), (0, 1, 2), (0, 2), (1, 2, 0), ())


def _must_fail(t, wrong, oracle_lib_path, swap=None):
    """``compare_dst`` of trial ``t`` given the expected output of ``wrong``
    (same inputs: they are seeded by flavour and index alone)."""
    case = fu.host_case(t, oracle_lib_path)
    bad = fu.host_case(wrong, oracle_lib_path)
    assert all(np.array_equal(a, b) for ra, rb in zip(case.srcs, bad.srcs)
               for a, b in zip(ra, rb))
    exp = bad.exp
    if swap is not None:
        c = swap
        exp = [row[:c] + [row[c + 1], row[c]] + row[c + 2:] for row in exp]
    fu.compare_dst(t, case, fu.as_got(t, case.exp))   # the right one passes
    with pytest.raises(AssertionError):
        fu.compare_dst(t, case, fu.as_got(t, exp))


def test_checker_sees_swapped_output_axes(oracle_lib_path):
    t = fu.Trial("plain", 0, CFG, (8, 1), 2)
    # (1, 2, 0) -> (1, 0, 2): the same local elements in another order
    wrong = t._replace(cfg=CFG[:5] + ((1, 0, 2),) + CFG[6:])
    _must_fail(t, wrong, oracle_lib_path)


def test_checker_sees_keep_bound_off_by_one(oracle_lib_path):
    t = fu.Trial("keep", 0, CFG, (4, 1), 2, keep=((7, 2), None, (6, 0)))
    for wrong_keep in (((8, 2), None, (6, 0)), ((7, 1), None, (6, 0)),
                       ((7, 2), None, (5, 0))):
        _must_fail(t, t._replace(keep=wrong_keep), oracle_lib_path)
    none = t._replace(fill=native.FILL_NONE)
    _must_fail(none, none._replace(keep=((7, 2), None, (7, 0))),
               oracle_lib_path)


def test_checker_sees_alpha_rounded_to_f32(oracle_lib_path):
    alpha = 1.0 / 3.0
    t = fu.Trial("scale", 0, CFG, "f64", 1, alpha=alpha)
    wrong = t._replace(alpha=float(np.float32(alpha)))
    assert wrong.alpha != alpha
    _must_fail(t, wrong, oracle_lib_path)


def test_checker_sees_exchanged_split_components(oracle_lib_path):
    t = fu.Trial("split", 0, CFG, 8, 3)
    _must_fail(t, t, oracle_lib_path, swap=1)


def test_checker_sees_lead_and_guard_writes(oracle_lib_path):
    t = fu.Trial("plain", 0, CFG, (8, 1), 2, lead=("dst", 1))
    case = fu.host_case(t, oracle_lib_path)
    for pos in (0, -1):   # first lead byte of field 1, last guard byte
        got = fu.as_got(t, case.exp)
        got[0][1][pos] = 0
        with pytest.raises(AssertionError):
            fu.compare_dst(t, case, got)
