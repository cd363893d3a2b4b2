"""Fuzz of grouped and truncated split / join transposes on one MI355X: 24
seeded trials each of a flagged split, a flagged join, a split with a keep
set, a join with one, and a scaled join with one, over random process grids
of up to 8 ranks run on ONE GPU (``soa_group_gpu_util.run_hop``: rows through
the query, results against the masked and scaled oracle, staging against the
n-field host run, guards)."""

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from soa_group_gpu_util import run_hop  # noqa: E402
from soa_keep_fuzz_util import draw, trial_ids  # noqa: E402

TRIALS = 24


@pytest.mark.parametrize("flavour,index", trial_ids(TRIALS),
                         ids=lambda v: str(v))
def test_fuzz_grouped_and_truncated_soa(flavour, index, oracle_lib_path):
    cfg, kind, n, direction, keep, fill, alpha = draw(flavour, index)
    run_hop(cfg, kind, n, direction, oracle_lib_path, keep=keep, fill=fill,
            alpha=alpha)
