"""-m gpu: validity masks through gdf_hash_partition on every route that moves them -- direct-generic, direct-fast, tile, two-level
and apply-map.  Output masks start as 0xff inside a larger 0xff allocation (hash_partition_gpu.OutMask): the library has to clear
them, may clear up to the next multiple of 4 bytes, and must leave everything beyond alone; bits from n on are 0.  A mask travels
only when both sides carry one; a column masked on one side only moves its data and nothing else is written (null_count
included).  A null key is partitioned by its stored bytes -- the verifier hashes what the column holds."""
import numpy as np
import pytest

import hash_partition_cases as hp
from hash_partition_gpu import run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", hp.MASK_CASES, ids=repr)
def test_masks(gdf, force_path, case):
    run_case(gdf, force_path, case)


def test_masks_one_level_and_two_levels_agree(gdf, force_path):
    case = next(c for c in hp.MASK_CASES if c.id == "masks-two-level-fast")
    two = run_case(gdf, force_path, case)
    one = run_case(gdf, force_path, case, forced={"GDF_HP_ONE_LEVEL": "1"}, expect=hp.notes_of(hp.DIRECT_FAST, 8, 1, 129))
    assert np.array_equal(one, two)
