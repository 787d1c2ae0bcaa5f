"""Points per LDS stage of the report kernels: the one formula of cloudini_amd/csrc/stage1_report.h (report_stage_points)
against the three it replaced, which stood in audit_kernels.hip, sweep_kernels.hip and mode_kernels.hip. The library offers no
way to the function without a device, so the formulas are restated here in integer arithmetic and a few values are pinned."""
import pytest

STAGED_STEP = 127      # kReportStagedStep
BLOCK_POINTS = 1024    # kReportBlockPoints; the mode kernel's thread count is the same number


def report_stage_points(point_step, lds_bytes, lead_points, cap, granule):
    """Mirrors the three lines of the body of `inline uint32_t report_stage_points(...)` in cloudini_amd/csrc/stage1_report.h
    (lines 49-53 when this was written; the function's name is the anchor): `fit = lds_bytes / point_step - lead_points`,
    capped, else rounded down to the granule."""
    if point_step == 0 or point_step > STAGED_STEP:
        return 0
    fit = lds_bytes // point_step - lead_points
    return cap if fit >= cap else (fit // granule) * granule


def audit_stage_points(point_step):
    """Both buffers' stages share (65536 - 256) bytes; lanes take points 256 apart."""
    if point_step == 0 or point_step > STAGED_STEP:
        return 0
    fit = ((65536 - 256) // 2 - 32) // point_step
    return BLOCK_POINTS if fit >= BLOCK_POINTS else (fit // 256) * 256


def sweep_stage_points(point_step):
    """One of the points that fit is the predecessor."""
    if point_step == 0 or point_step > STAGED_STEP:
        return 0
    fit = (40960 - 32) // point_step - 1
    return BLOCK_POINTS if fit >= BLOCK_POINTS else (fit // 256) * 256


def modes_stage_points(point_step):
    """Two of the points that fit are the predecessors; one value per lane, whole waves."""
    if point_step == 0 or point_step > STAGED_STEP:
        return 0
    fit = (40960 - 32) // point_step - 2
    return 1024 if fit >= 1024 else (fit // 64) * 64


KINDS = {"audit": (audit_stage_points, ((65536 - 256) // 2 - 32, 0, 1024, 256)),
         "sweep": (sweep_stage_points, (40960 - 32, 1, 1024, 256)),
         "modes": (modes_stage_points, (40960 - 32, 2, 1024, 64))}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_shared_formula_gives_the_values_of_the_one_it_replaced(kind):
    old, (lds_bytes, leads, cap, granule) = KINDS[kind]
    for step in range(0, 201):
        got = report_stage_points(step, lds_bytes, leads, cap, granule)
        assert got == old(step), (kind, step)
        assert (got == 0) == (step == 0 or step > STAGED_STEP), (kind, step)
        if got:
            # the stage, its predecessors and report_stage's slack of 32 bytes fit the budget; a stage is at least one granule
            assert (got + leads) * step <= lds_bytes and got >= granule and got <= cap and (got == cap or got % granule == 0)


def test_pinned_values():
    table = {kind: [report_stage_points(s, *args) for s in (1, 16, 19, 31, 32, 39, 40, 47, 64, 100, 127, 128, 200)]
             for kind, (_old, args) in KINDS.items()}
    assert table == {"audit": [1024, 1024, 1024, 1024, 768, 768, 768, 512, 256, 256, 256, 0, 0],
                     "sweep": [1024, 1024, 1024, 1024, 1024, 1024, 768, 768, 512, 256, 256, 0, 0],
                     "modes": [1024, 1024, 1024, 1024, 1024, 1024, 960, 832, 576, 384, 320, 0, 0]}
