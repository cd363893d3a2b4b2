"""What the default trial lists of the multi-rank fuzz (fuzz_util.py,
test_gpu_fuzz_multirank.py) reach, pinned on the CPU so that the fuzz cannot
hide a gap: per flavour every kernel family it has, and enough trials with
several ranks, an empty rank, every ``nd``, a permuted source pencil, extra
dims, and tile descriptors with two batch axes, with the
destination-contiguous axis behind a batch axis, and with more than one tile.

Host queries only: native plans, ``stage_launches`` and the kind queries with
fake aligned or one-scalar-off pointers.  ``fuzz_util.check_selection`` also
asserts on the way that every trial's launch rows agree with the
per-descriptor queries."""

import collections
import os

import pytest

import fuzz_util as fu

native = pytest.importorskip("pencilarrays_amd.native")

if not os.path.exists(native.lib_path()):
    pytest.skip("libpencilhip.so not built", allow_module_level=True)

K = native
PLAIN = {K.KERNEL_LINEAR, K.KERNEL_TILE, K.KERNEL_TILE_VS, K.KERNEL_TILE_PK,
         K.KERNEL_TILE_WIDE, K.KERNEL_GENERIC}
CVT = {K.KERNEL_CVT_LINEAR, K.KERNEL_CVT_TILE, K.KERNEL_CVT_GENERIC}
SOA = {K.KERNEL_SOA_LINEAR, K.KERNEL_SOA_TILE, K.KERNEL_SOA_GENERIC}
# the kernel kinds every flavour's list must launch
FAMILIES = {
    "plain": PLAIN,
    "keep": PLAIN | {K.KERNEL_FILL},
    "wire": CVT,
    "wire_group": CVT,
    "scale": {K.KERNEL_SCALE_LINEAR, K.KERNEL_SCALE_TILE,
              K.KERNEL_SCALE_GENERIC},
    "split": SOA,    # pa_transpose_pack_split / _local_split
    "join": SOA,     # pa_transpose_local_join / _unpack_join
}
# and those it must launch as grouped rows
GROUPED = {"wire_group": {K.KERNEL_CVT_LINEAR, K.KERNEL_CVT_TILE}}


def report(flavour):
    """``(histogram of (kind, grouped) rows, largest grouped row, counts of
    trials with each property)`` over the flavour's default list."""
    hist, stats, biggest = collections.Counter(), collections.Counter(), 0
    trials = [fu.draw_cfg(flavour, i)
              for i in range(fu.DEFAULT_TRIALS[flavour])]
    for t in trials:
        rows, _ = fu.host_rows(t)
        for l in rows:
            hist[(l.kind, l.grouped)] += 1
            if l.grouped:
                biggest = max(biggest, l.entries)
        dims, _, _, pi, _, _, extra = t.cfg
        tiles = fu.tile_descriptors(t)
        stats["ranks>=2"] += fu.nranks(t) >= 2
        stats["empty rank"] += fu.has_empty_rank(t)
        stats[f"nd={len(dims)}"] += 1
        stats["permuted input"] += pi != tuple(range(len(dims)))
        stats["extra dims"] += bool(extra)
        stats["tile, >=2 batch axes"] += any(len(d) >= 4 for d, _, _ in tiles)
        stats["tile, ta != 1"] += any(ta != 1 for _, ta, _ in tiles)
        stats["tile axis of >=2 tiles"] += any(nt >= 2 for _, _, nt in tiles)
    return hist, biggest, stats, len(trials)


def format_report(flavour):
    hist, biggest, stats, ntrials = report(flavour)
    rows = ", ".join(f"{K.KERNEL_NAMES[k]}{'/grouped' if g else ''}: {c}"
                     for (k, g), c in sorted(hist.items()))
    return (f"{flavour}: {ntrials} trials; rows {rows}; largest group "
            f"{biggest}; " + ", ".join(f"{k}: {v}"
                                       for k, v in sorted(stats.items())))


@pytest.mark.parametrize("flavour", fu.FLAVOURS)
def test_default_trials_reach_every_family_and_shape_class(flavour):
    hist, biggest, stats, ntrials = report(flavour)
    print(format_report(flavour))
    missing = FAMILIES[flavour] - {k for k, _ in hist}
    assert not missing, [K.KERNEL_NAMES[k] for k in missing]
    missing = GROUPED.get(flavour, set()) - {k for k, g in hist if g}
    assert not missing, [K.KERNEL_NAMES[k] for k in missing]
    if flavour == "plain":
        assert biggest >= 3
    assert 3 * stats["ranks>=2"] >= ntrials, stats
    assert stats["empty rank"] >= 2, stats
    for nd in (2, 4, 5):
        assert stats[f"nd={nd}"] >= 3, stats
    assert stats["permuted input"] >= 4, stats
    assert stats["extra dims"] >= 3, stats
    assert stats["tile, >=2 batch axes"] >= 3, stats
    assert stats["tile, ta != 1"] >= 3, stats
    assert stats["tile axis of >=2 tiles"] >= 3, stats


def test_trials_are_reproducible_and_within_the_caps():
    import math
    for flavour in fu.FLAVOURS:
        for world1 in (False, True):
            for i in range(fu.trial_count(flavour, world1)):
                t = fu.draw_cfg(flavour, i, world1)
                assert t == fu.draw_cfg(flavour, i, world1)
                dims, pdims, _, _, _, _, extra = t.cfg
                assert 2 <= len(dims) <= 5
                assert math.prod(dims) * math.prod(extra or (1,)) <= \
                    fu.MAX_ELEMS
                assert fu.nranks(t) <= (1 if world1 else fu.MAX_RANKS)
                assert not t.aliased or flavour in fu.CAN_ALIAS
                if t.keep is not None:
                    assert all(k is None or (k[0] >= 0 and k[1] >= 0 and
                                             k[0] + k[1] <= N)
                               for k, N in zip(t.keep, dims))
    # the forced keep sets: nothing kept, everything kept
    keeps = [fu.draw_cfg("keep", i) for i in range(fu.DEFAULT_TRIALS["keep"])]
    assert any((0, 0) in t.keep for t in keeps)
    assert any(all(k is None or sum(k) == N
                   for k, N in zip(t.keep, t.cfg[0])) for t in keeps)
