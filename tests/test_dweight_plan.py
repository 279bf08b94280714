"""The block-shape plan of the grouped weight-gradient launch (g2048_dweight_jobs_plan, csrc/g2048_dweight.hip): host arithmetic, CPU only.

A launch's jobs are cut into [256 x 256] cells; the plan says how many leading cells of each job run as one [256 x 256] block (the rest as
four [128 x 128] blocks each).  One workgroup occupies a CU, so with W = sum(cells x slices) workgroups of big blocks on `cus` CUs the
rule is: W // cus whole rounds of big blocks first; the W % cus left over as 4 x as many [128 x 128] workgroups when that is at most two
rounds of the chip, else as big blocks too; less than one round of big blocks: all [128 x 128]."""
import pytest

S = 8
LAYER = [(256, 1024, S), (1024, 256, S), (256, 256, S), (768, 256, S)]
UPDATE = [(512, 256, S)] + LAYER * 3  # the default model's update: K/V of the CLS-only last layer, then three full layers
CELLS = [2] + [4, 4, 1, 3] * 3


def _plan(shapes, big_cells=-1, cus=0):
    from src.g2048 import native as nv

    return nv.dweight_jobs_plan(shapes, big_cells, cus)


def test_update_job_list_on_256_cus():
    n_big = _plan(UPDATE, cus=256)
    assert sum(CELLS) * S == 304                             # 1.19 rounds of big blocks
    assert sum(n_big) * S == 256                             # one full round of them ...
    assert 4 * (sum(CELLS) - sum(n_big)) * S == 192          # ... and the rest as [128 x 128] blocks, less than a round
    assert n_big == CELLS[:10] + [2, 0, 0]                   # dealt in job order: the last jobs take the small blocks, one job is mixed


@pytest.mark.parametrize("cus,want", [(304, CELLS), (64, CELLS), (512, [0] * 13), (100, CELLS[:12] + [2])])
def test_rule(cus, want):
    # 304: exactly one round.  64: 4 rounds + 48 left, 192 small workgroups > 2 x 64: all big.  512: less than a round: all small.
    # 100: 3 rounds + 4 workgroups left -> 300 // 8 = 37 cells big, one cell small
    assert _plan(UPDATE, cus=cus) == want


def test_explicit_counts_and_ineligible_jobs():
    shapes = [(384, 128, S), (256, 256, 16), (128, 256, S), (512, 512, S)]
    assert _plan(shapes, 1000) == [0, 1, 0, 4]               # N or K no multiple of 256: no cells
    assert _plan(shapes, 3) == [0, 1, 0, 2]
    assert _plan(shapes, 0) == [0, 0, 0, 0]
    assert _plan(shapes, cus=16) == [0, 1, 0, 4]             # 16 + 32 workgroups = 3 rounds of 16


def test_refusals():
    from src.g2048 import native as nv

    with pytest.raises(nv.NativeError):
        _plan(UPDATE, cus=0)                                 # the launch's own choice needs a CU count
    with pytest.raises(nv.NativeError):
        _plan(UPDATE * 2, 0)                                 # more than G2048_DWG_MAX_JOBS
