"""Property fuzz of every plan flavour across random process grids on one
MI355X, bit for bit against host references (fuzz_util.py).

- Stage-sim tests, one case per trial: plain n-field plans (elem_dims and
  aliased plans among them), keep, wire ungrouped and grouped, scale with and
  without keep, split, join.  Every rank of a random grid of up to 8 ranks
  runs on the one GPU through the stage API, device slice copies at the
  ``peer_message`` ranges standing in for the exchange.
- A world-1 group through the Python classes: ``Transposition`` /
  ``MultiTransposition`` with ``keep=`` / ``wire_dtype=`` / ``wire_grouped=``
  / ``scale=``, ``SplitTransposition`` / ``JoinTransposition``, in place where
  the flavour allows it, on the pooled staging, each trial run twice.

A trial is drawn from its flavour and index alone
(``fuzz_util.draw_cfg(flavour, index)``, the case's pytest id), and every
assertion message carries the whole trial.  Each case first asserts with the
real device pointers that ``stage_launches`` agrees with the per-descriptor
kind queries, then launches.  Destinations and staging are 0xAB-filled with
256-byte guards; whole buffers are compared.
``PENCILHIP_FUZZ_MULTIRANK_TRIALS=N`` runs N trials per flavour for a soak;
tests/test_fuzz_coverage.py pins what the default lists reach."""

import pytest

import fuzz_util as fu

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)


def _trials(flavour, world1=False):
    return pytest.mark.parametrize(
        "index", range(fu.trial_count(flavour, world1)),
        ids=lambda i: f"{flavour}-{i}")


def _stage(flavour, index, oracle_lib_path):
    fu.run_stage_fuzz(fu.draw_cfg(flavour, index), oracle_lib_path)


def _world1(flavour, index, oracle_lib_path):
    fu.run_world1_fuzz(fu.draw_cfg(flavour, index, world1=True),
                       oracle_lib_path)


@_trials("plain")
def test_stage_plain(index, oracle_lib_path):
    _stage("plain", index, oracle_lib_path)


@_trials("keep")
def test_stage_keep(index, oracle_lib_path):
    _stage("keep", index, oracle_lib_path)


@_trials("wire")
def test_stage_wire(index, oracle_lib_path):
    _stage("wire", index, oracle_lib_path)


@_trials("wire_group")
def test_stage_wire_grouped(index, oracle_lib_path):
    _stage("wire_group", index, oracle_lib_path)


@_trials("scale")
def test_stage_scale(index, oracle_lib_path):
    _stage("scale", index, oracle_lib_path)


@_trials("split")
def test_stage_split(index, oracle_lib_path):
    _stage("split", index, oracle_lib_path)


@_trials("join")
def test_stage_join(index, oracle_lib_path):
    _stage("join", index, oracle_lib_path)


@_trials("plain", world1=True)
def test_world1_plain(index, oracle_lib_path):
    _world1("plain", index, oracle_lib_path)


@_trials("keep", world1=True)
def test_world1_keep(index, oracle_lib_path):
    _world1("keep", index, oracle_lib_path)


@_trials("wire", world1=True)
def test_world1_wire(index, oracle_lib_path):
    _world1("wire", index, oracle_lib_path)


@_trials("wire_group", world1=True)
def test_world1_wire_grouped(index, oracle_lib_path):
    _world1("wire_group", index, oracle_lib_path)


@_trials("scale", world1=True)
def test_world1_scale(index, oracle_lib_path):
    _world1("scale", index, oracle_lib_path)


@_trials("split", world1=True)
def test_world1_split(index, oracle_lib_path):
    _world1("split", index, oracle_lib_path)


@_trials("join", world1=True)
def test_world1_join(index, oracle_lib_path):
    _world1("join", index, oracle_lib_path)
