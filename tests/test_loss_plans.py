"""ga_loss_lds_plan on the host (no GPU): the LDS plan every loss launch takes — whether the guided columns of A are resident
(`use_gcol`) and how many rows of A a softmax-statistics pass stages (`stage_rows`) — over a sweep of the sizes the launches
serve, against the kernels' LDS layout restated here; and the coverage condition of tests/test_loss_plans_gpu.py: the plans its
case lists declare include every plan class the sweep finds reachable."""
import ctypes

import pytest

import test_loss_plans_gpu as gpu_cases
from test_abi import lib  # noqa: F401  (the fixture: builds the library when it is missing)

ROW_BYTES = (1576 + 15) // 16 * 16                # one staged ga_image_loss_t row
REL_FRONT_BYTES = ROW_BYTES + 336 + 960           # + the relation row and the relation state (RelLds) of the *_rel_* launches
LDS_LIMIT = 160 * 1024


def table_bytes(kind, npix, Kt, slots, w_lds, rel):
    """The kernels' fixed tables (csrc/smooth_loss.hip: loss_forward / loss_backward): mx, sm, M, Pn (+ G, dot, colmap and dS
    [slots][npix] in the backward), 16 floats of scratch, W [npix] when the strict table is reserved, sm2 [npix] of the relation
    launches."""
    if kind == gpu_cases.BWD:
        floats = 6 * npix + 16 + ((Kt + 3) & ~3) + slots * npix
    else:
        floats = 4 * npix + 16
    return 4 * (floats + (npix if w_lds else 0) + (npix if rel else 0))


@pytest.fixture(scope="module")
def sweep(lib):  # noqa: F811
    return gpu_cases.sweep_plans(lib)


def test_query_returns_the_launch_shape_error_or_a_plan(sweep):
    assert len(sweep) > 100000
    served = 0
    for (kind, table, rel, images, res, Kt, slots, Q, strict, addr), (rc, gcol, rows, lds) in sweep.items():
        npix = res * res
        what = (kind, table, rel, images, res, Kt, slots, Q, strict, addr, rc, gcol, rows, lds)
        w_lds = 1 if table else strict
        n_slots = slots + (Q if rel else 0)
        tables = table_bytes(kind, npix, Kt, n_slots, w_lds, rel)
        if rc != 0:
            # the launches' own refusals: the table capacities, or fixed tables beyond the 150 KB budget
            assert rc == -2, what
            assert ((table and slots * npix > 24576) or (rel and n_slots * npix > 24576) or tables > 150 * 1024), what
            continue
        served += 1
        assert gcol in (0, 1) and rows >= 0, what
        assert lds <= LDS_LIMIT, what
        assert rows % 4 == 0, what
        assert rows <= max(256, (npix + 3) & ~3), what
        assert rows in (0, 32, 64, 128, 256) or (npix < 256 and rows == (npix + 3) & ~3), what
        if addr % 16:
            assert rows == 0, what
        if images > 1 and (npix * Kt) % 4:
            assert rows == 0, what
        # the staging area (16-byte aligned: up to 16 bytes of slack) fits behind the descriptor rows, the tables and the columns
        front = REL_FRONT_BYTES if rel else (ROW_BYTES if table else 0)
        assert front + tables + (4 * n_slots * npix if gcol else 0) + 16 + 4 * rows * Kt <= lds, what
    assert served > 50000


def test_argument_errors(lib):  # noqa: F811
    g, r, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    out = (ctypes.byref(g), ctypes.byref(r), ctypes.byref(n))
    p = ctypes.c_void_p(4096)
    assert lib.ga_loss_lds_plan(gpu_cases.BWD, 0, 0, 1, 16, 77, 3, 0, 0, p, *out) == 0 and (g.value, r.value) == (1, 256)
    assert lib.ga_loss_lds_plan(gpu_cases.BWD, 0, 0, 1, 16, 77, 3, 0, 0, None, *out) == -1
    assert lib.ga_loss_lds_plan(gpu_cases.BWD, 0, 0, 1, 16, 77, 3, 0, 0, p, None, out[1], out[2]) == -1
    assert lib.ga_loss_lds_plan(gpu_cases.BWD, 0, 0, 1, 65, 77, 3, 0, 0, p, *out) == -2       # res > 64
    assert lib.ga_loss_lds_plan(gpu_cases.BWD, 0, 0, 1, 16, 77, 33, 0, 0, p, *out) == -2      # more than 32 token slots
    assert lib.ga_loss_lds_plan(gpu_cases.BWD, 0, 0, 65, 16, 77, 3, 0, 0, p, *out) == -2      # more than GA_MAX_IMAGES
    assert lib.ga_loss_lds_plan(gpu_cases.BWD, 0, 0, 1, 64, 77, 3, 0, 0, p, *out) == 0
    assert lib.ga_loss_lds_plan(gpu_cases.BWD, 0, 0, 1, 64, 77, 4, 0, 0, p, *out) == -2       # the tables alone exceed the budget
    assert lib.ga_loss_lds_plan(gpu_cases.BWD, 1, 0, 1, 32, 77, 25, 0, 0, p, *out) == -2      # T_max * res^2 > 24576
    assert lib.ga_loss_lds_plan(gpu_cases.BWD, 1, 1, 1, 32, 77, 16, 33, 0, p, *out) == -2     # Q_max > 32
    assert lib.ga_loss_lds_plan(gpu_cases.FWD, 1, 0, 1, 16, 77, 3, 0, 0, p, *out) == -6       # no solo forward in table form
    assert lib.ga_loss_lds_plan(gpu_cases.FWD, 0, 0, 3, 16, 77, 3, 0, 0, p, *out) == -6
    assert lib.ga_loss_lds_plan(gpu_cases.AGG_FWD, 0, 1, 1, 16, 77, 3, 4, 0, p, *out) == -6   # relations need the table form
    assert lib.ga_loss_lds_plan(7, 0, 0, 1, 16, 77, 3, 0, 0, p, *out) == -6


def test_wrapper_reports_the_plan_or_raises():
    from guided_attention_amd import ops
    assert tuple(ops.loss_lds_plan("bwd", 16, 77, 3))[:2] == (1, 256)
    assert tuple(ops.loss_lds_plan("bwd", 16, 77, 3, A=4100))[:2] == (1, 0)
    assert tuple(ops.loss_lds_plan("bwd", 32, 77, 16, images=3, table=True))[:2] == (0, 128)      # an SDXL table of 16 tokens
    assert tuple(ops.loss_lds_plan("agg_fwd", 32, 77, 16, images=3, table=True))[:2] == (0, 256)
    assert tuple(ops.loss_lds_plan("bwd", 32, 77, 16, images=3, table=True, Q_max=4))[:2] == (0, 64)
    assert tuple(ops.loss_lds_plan("bwd", 5, 77, 3, images=3))[:2] == (1, 0)                       # 25 * 77 is no multiple of 4
    with pytest.raises(ops.GaError, match="ga_loss_lds_plan"):
        ops.loss_lds_plan("bwd", 64, 77, 4)


def test_every_declared_plan_is_what_the_query_reports():
    """The case lists of the GPU file against the query, here as well: a planner change shows without a GPU."""
    from guided_attention_amd import ops
    declared = gpu_cases.declared_plans()
    assert len(declared) > 60
    for what, kind, kw, plan in declared:
        gpu_cases.expect_plan(ops, what, kind, plan, **kw)


def test_declared_plans_cover_every_reachable_class(sweep):
    gpu_cases.assert_coverage(sweep)
