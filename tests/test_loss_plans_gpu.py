"""The loss kernels of csrc/smooth_loss.hip (solo, batched, image-table and relation forms, forward and backward) on every LDS
plan the host can choose, on the MI355X.  A launch's plan is (`use_gcol`: the guided columns of A resident in LDS or re-read
from global memory, `stage_rows`: rows of A staged through LDS per pass of the softmax statistics, 0: none); it follows from res,
Kt, the token slots, the strict table and the alignment of A.  Every case below names the plan it runs, forward and backward,
and asserts that ops.loss_lds_plan (the code the launches take their plan from) reports it before launching.

  (a) the solo kernels against the float64 closed form (oracle.loss.loss_and_grad_numpy), f32 / f16 / bf16 head-maps;
  (b) the same input under different plans gives the same bits: aligned against misaligned maps, image tables of growing
      capacity, batched launches, relation tables of growing Q_max — each image also against the solo entry points;
  (c) the table, batched and relation forms against float64 away from plan (1, 256), and the batched launches of ragged maps
      that stage nothing.

Bounds, everywhere: 5e-5 of the gradient's maximum for dA, rtol 5e-5 for the loss and the term columns (atol 1e-6 on the terms)
— the bounds of test_smooth_loss_other_resolutions.  The broadcast map dP_bcast is dA * scale exactly in f32 and within the
16-bit formats' rounding (2e-3 / 1.6e-2 of the maximum) in f16 / bf16.  Every test prints its figures ([measured] lines).

The case lists are module constants without device state: tests/test_loss_plans.py imports them on a machine without a GPU to
check them against the query and to assert, as this file does, that they cover every plan class the query finds reachable."""
import ctypes

import numpy as np
import pytest
import torch

import hashrand
from oracle import loss as oloss

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
TOL = {"f32": 2e-5, "f16": 2e-3, "bf16": 1.6e-2}       # of the tensor's maximum: tests/test_kernels_gpu.py
GRAD_TOL, RTOL, ATOL = 5e-5, 5e-5, 1e-6
SCALE = .125                                           # bcast_scale: a power of two, dA * SCALE is exact in every format's range
FWD, AGG_FWD, BWD = 0, 1, 2                            # `kind` of ga_loss_lds_plan (include/ga_hip.h)
KIND_NAME = {FWD: "fwd", AGG_FWD: "agg_fwd", BWD: "bwd"}
TERM_KEYS = ("max", "col", "row", "inside", "outside", "token_loss", "unscaled")


def _box(i, g, sub):
    return {"index": i, "kind": "BOX", "geom": g, "subprompt": sub}


def _coor(i, g, sub):
    return {"index": i, "kind": "COOR", "geom": g, "subprompt": sub}


def entries_of(T):
    """T guided tokens in distinct columns (index 2 + t), BOX and COOR mixed, two tokens per sub-prompt.  The boxes are
    distinct, .45 x .5 of the image: shrunk by .15 per side they still span .315 x .35, more than the pixel pitch of every
    map from 5 x 5 up, and at 2 x 2 the first box holds the pixel centre (.25, .25)."""
    return [_coor(2 + t, (.2 + .02 * t, .3 + .015 * t), f"w{t // 2}") if t % 3 == 1 else
            _box(2 + t, (.05 + .015 * t, .1 + .01 * (t % 7), .45, .5), f"w{t // 2}") for t in range(T)]


# ----------------------------------------------------------------------------------------------------------- the case lists
FLAT = .05   # head-maps this flat (100 * A varies by +-0.1 along a row) give every element of a row weight in its softmax sum


def _solo(name, res, Kt, T, fwd, bwd, strict=False, avg=False, last=None, misaligned=False, sharp=3.0):
    """One argument-form case: the solo forward (`fwd`) and backward (`bwd`) plans on the case's map; the fused aggregate
    forward writes A into a buffer of its own (aligned): it runs `fwd` too unless the case's map is misaligned.  `sharp`: the
    head-maps are softmax(sharp * noise) — 3: near-one-hot rows after the x100, FLAT: every column counts."""
    return dict(name=name, res=res, Kt=Kt, T=T, fwd=fwd, bwd=bwd, strict=strict, avg=avg, last=Kt - 1 if last is None else last,
                misaligned=misaligned, sharp=sharp)


SOLO_CASES = [
    # argument form, Kt = 77
    _solo("r16_T3", 16, 77, 3, (1, 256), (1, 256)),                       # the plan every earlier fp64 comparison ran
    _solo("r24_T16", 24, 77, 16, (1, 256), (0, 256)),                     # SD-2.1 768: a table of 16 tokens
    _solo("r24_T28", 24, 77, 28, (1, 256), (0, 128)),                     # ... of 32
    _solo("r32_T8", 32, 77, 8, (1, 256), (0, 256)),                       # SDXL: 5 to 8 guided tokens
    _solo("r32_T24", 32, 77, 24, (0, 256), (0, 64)),
    _solo("r32_T28", 32, 77, 28, (0, 256), (0, 32)),
    _solo("r32_T30", 32, 77, 30, (0, 256), (0, 0)),
    _solo("r48_T3", 48, 77, 3, (1, 256), (0, 128)),
    _solo("r64_T1", 64, 77, 1, (0, 256), (0, 64)),
    _solo("r64_T1_strict", 64, 77, 1, (0, 128), (0, 64), strict=True),   # the strict table pushes the forward to 128 rows
    _solo("r32_k128_T2", 32, 128, 2, (1, 128), (1, 128)),                 # resident columns next to a half-size staging area
    # small and ragged maps: the padded stage_rows and the scalar tail of the staging loop (n = npix * Kt).  The tail's elements
    # are the last pixel's last columns: the slice reaches them (last = Kt at Kt = 77) and the maps are flat, so that a tail
    # element that is not staged moves its row's sum (on near-one-hot rows a lost column of e^-20 would go unseen)
    _solo("r2_k8", 2, 8, 2, (1, 4), (1, 4)),
    _solo("r5_k77", 5, 77, 3, (1, 28), (1, 28), last=77, sharp=FLAT),     # n % 4 == 1: the tail is column 76 of pixel 24
    _solo("r7_k78", 7, 78, 4, (1, 52), (1, 52), avg=True, sharp=FLAT),    # n % 4 == 2: columns 76, 77; sub_prompt_avg_within
    _solo("r8_k77", 8, 77, 3, (1, 64), (1, 64), strict=True),
    _solo("r6_k128", 6, 128, 3, (1, 36), (1, 36), last=40),               # the text slice ends early
    # a map one float into a larger buffer: nothing is staged
    _solo("r16_T3_misaligned", 16, 77, 3, (1, 0), (1, 0), misaligned=True),
    _solo("r32_T24_misaligned", 32, 77, 24, (0, 0), (0, 0), misaligned=True),
]

# image rows of at most 4 tokens: (entries, hyper-parameters over the defaults, last of the text slice, sub_prompt_avg_within)
TABLE_ROWS = [
    ([_box(2, (.6, .3, .4, .55), "robot"), _coor(5, (.25, .7), "blue vase"), _box(6, (.2, .3, .4, .55), "blue vase"),
      _box(9, (.05, .5, .9, .45), "sofa")], {}, 76, False),
    ([_box(3, (.1, .2, .5, .6), "cat"), _coor(7, (.3, .7), "ball")], {"strict": True, "shrink_factor": .1}, 76, False),
    ([], {}, 76, False),                                                                              # not guided: T = 0
    ([_coor(2, (.5, .5), "dog"), _box(4, (.05, .5, .9, .45), "dog"), _box(8, (.3, .1, .5, .5), "dog")],
     {"inside_loss_scale": .5, "outside_loss_scale": .1, "bb_center_weight": .2}, 40, True),        # the slice ends early
    ([_box(2, (.3, .2, .5, .6), "robot"), _coor(4, (.6, .4), "vase")], {}, 76, False),                # takes no update: dloss = 0
]
TABLE_DLOSS = [1.5, 2.5, 1.0, .75, 0.0]
# res -> [(T_max, forward plan, backward plan)]: the first capacity is the one the others are compared with
TABLE_CASES = {
    32: [(4, (1, 256), (1, 256)), (8, (1, 256), (0, 256)), (12, (1, 256), (0, 128)), (24, (0, 256), (0, 64))],
    40: [(4, (1, 256), (0, 256)), (14, (0, 256), (0, 32))],
    48: [(4, (0, 256), (0, 128)), (8, (0, 256), (0, 32)), (9, (0, 256), (0, 0))],
}

# batched argument form, S = 3 at res 32: (T, forward plan, backward plan, backward plan on a misaligned A)
BATCHED_CASES = [(8, (1, 256), (0, 256), (0, 0)), (14, (1, 256), (0, 128), (0, 0)), (24, (0, 256), (0, 64), (0, 0))]

# relation tables of T_max 4, S = 3: res -> [(Q_max, forward plan, backward plan)]
REL_ENTRIES = [_box(3, (.1, .2, .6, .6), "cat"), _coor(8, (.7, .3), "ball")]      # slice index 2 is a guided column too
REL_RELATIONS = [([2, 5], [0]), ([5], [2])]                                       # three distinct columns
REL_CASES = {
    16: [(4, (1, 256), (1, 256)), (8, (1, 256), (1, 256)), (16, (1, 256), (1, 256))],
    32: [(4, (1, 256), (0, 256)), (8, (1, 256), (0, 128)), (16, (0, 256), (0, 64))],
}
# one image at res 15 (225 pixels: padded to 228 staged rows): (T_max, Q_max, forward plan, backward plan) — 24 + 16 slots are the
# one way to a plan without resident columns on a map below 256 pixels
REL_SMALL_RES = 15
REL_SMALL_CASES = [(4, 4, (1, 228), (1, 228)), (24, 16, (1, 228), (0, 228))]

# (c) S = 3 at res 32, away from (1, 256): form -> (slots, Q_max or None, forward plan, backward plan)
FP64_FORMS = {"table": (16, None, (0, 256), (0, 128)), "batched": (14, None, (1, 256), (0, 128)),
              "relation": (16, 4, (0, 256), (0, 64))}
# batched launches of ragged maps (npix * Kt no multiple of 4: nothing is staged), S = 3, Kt = 77: res -> (plan, the solo plan)
RAGGED_CASES = {5: ((1, 0), (1, 28)), 7: ((1, 0), (1, 52))}


def declared_plans():
    """[(what, kind, keyword arguments of ops.loss_lds_plan, (use_gcol, stage_rows))] of every case above."""
    out = []
    for c in SOLO_CASES:
        kw = dict(res=c["res"], Kt=c["Kt"], slots=c["T"], strict=c["strict"])
        mis = dict(kw, A=4100) if c["misaligned"] else kw
        out += [(c["name"], FWD, mis, c["fwd"]), (c["name"], BWD, mis, c["bwd"])]
        if not c["misaligned"]:
            out.append((c["name"], AGG_FWD, kw, c["fwd"]))
    for res, caps in TABLE_CASES.items():
        for T_max, fwd, bwd in caps:
            kw = dict(res=res, Kt=77, slots=T_max, images=len(TABLE_ROWS), table=True)
            out += [(f"table r{res} T_max {T_max}", AGG_FWD, kw, fwd), (f"table r{res} T_max {T_max}", BWD, kw, bwd)]
    for T, fwd, bwd, bwd_mis in BATCHED_CASES:
        kw = dict(res=32, Kt=77, slots=T, images=3)
        out += [(f"batched T {T}", AGG_FWD, kw, fwd), (f"batched T {T}", BWD, kw, bwd),
                (f"batched T {T} misaligned", BWD, dict(kw, A=4100), bwd_mis)]
    for res, qs in REL_CASES.items():
        for Q, fwd, bwd in qs:
            kw = dict(res=res, Kt=77, slots=4, images=3, table=True, Q_max=Q)
            out += [(f"relation r{res} Q_max {Q}", AGG_FWD, kw, fwd), (f"relation r{res} Q_max {Q}", BWD, kw, bwd)]
    for T_max, Q, fwd, bwd in REL_SMALL_CASES:
        kw = dict(res=REL_SMALL_RES, Kt=77, slots=T_max, images=1, table=True, Q_max=Q)
        out += [(f"relation r15 T_max {T_max} Q_max {Q}", AGG_FWD, kw, fwd), (f"relation r15 T_max {T_max} Q_max {Q}", BWD, kw, bwd)]
    for form, (slots, Q, fwd, bwd) in FP64_FORMS.items():
        kw = dict(res=32, Kt=77, slots=slots, images=3, table=form != "batched", Q_max=Q)
        out += [(f"fp64 {form}", AGG_FWD, kw, fwd), (f"fp64 {form}", BWD, kw, bwd)]
    for res, (plan, solo) in RAGGED_CASES.items():
        kw = dict(res=res, Kt=77, slots=3, images=3)
        out += [(f"ragged r{res}", AGG_FWD, kw, plan), (f"ragged r{res}", BWD, kw, plan),
                (f"ragged r{res} solo", FWD, dict(kw, images=1), solo), (f"ragged r{res} solo", BWD, dict(kw, images=1), solo)]
    return out


def expect_plan(ops, what, kind, plan, **kw):
    got = ops.loss_lds_plan(KIND_NAME[kind], **kw)
    assert (got.use_gcol, got.stage_rows) == tuple(plan), \
        f"the planner changed: update this case ({what}, {KIND_NAME[kind]}: declared {tuple(plan)}, the query reports {got})"
    return got


# ------------------------------------------------------------------------------------------------- the coverage condition
def plan_class(use_gcol, stage_rows, npix):
    """(use_gcol, stage_rows class): 0, 32, 64, 128, 256, or 'npix' — the map's pixels rounded up to 4, for maps below 256."""
    return use_gcol, ("npix" if stage_rows and npix < 256 else stage_rows)


_SWEEP = {}


def sweep_plans(lib):
    """The query over res 2 .. 64, Kt in {2, 8, 77, 78, 80, 128}, 1 .. 32 slots, both alignments, 1 and 3 images, every entry
    kind and form -> {(kind, table, relations, images, res, Kt, slots, Q_max, strict, address): (rc, use_gcol, stage_rows, lds)}."""
    if _SWEEP:
        return _SWEEP
    g, r, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    pg, pr, pn = ctypes.byref(g), ctypes.byref(r), ctypes.byref(n)
    fn = lib.ga_loss_lds_plan
    forms = [(FWD, 0, 0, 0, 0), (AGG_FWD, 0, 0, 0, 1), (BWD, 0, 0, 0, 0), (BWD, 0, 0, 0, 1), (AGG_FWD, 1, 0, 0, 0), (BWD, 1, 0, 0, 0),
             (AGG_FWD, 1, 1, 16, 0), (BWD, 1, 1, 16, 0)]
    for images in (1, 3):
        for kind, table, rel, Q, strict in forms:
            if kind == FWD and images != 1:
                continue
            for addr in (4096, 4100):
                p = ctypes.c_void_p(addr)
                for res in range(2, 65):
                    for Kt in (2, 8, 77, 78, 80, 128):
                        for slots in range(1, 33):
                            rc = fn(kind, table, rel, images, res, Kt, slots, Q, strict, p, pg, pr, pn)
                            _SWEEP[(kind, table, rel, images, res, Kt, slots, Q, strict, addr)] = (rc, g.value, r.value, n.value)
    return _SWEEP


def assert_coverage(sweep):
    """The declared plans include every use_gcol value crossed with every stage_rows class the sweep reaches."""
    reachable = {plan_class(gcol, rows, key[4] ** 2) for key, (rc, gcol, rows, _) in sweep.items() if rc == 0}
    declared = {plan_class(plan[0], plan[1], kw["res"] ** 2) for _, _, kw, plan in declared_plans()}
    assert {(1, 256), (0, 256), (0, 128), (0, 64), (0, 32), (0, 0), (1, 0), (1, "npix")} <= reachable, sorted(reachable, key=str)
    assert not {(1, 64), (1, 32)} & reachable          # 64 and 32 rows are what is left once the columns did not fit
    missing = reachable - declared
    assert not missing, f"no case runs under {sorted(missing, key=str)}: add one to tests/test_loss_plans_gpu.py"


# ------------------------------------------------------------------------------------------------------------ GPU helpers
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    return _ops


def softmax_maps(shape, seed, sharp=2.0):
    """Deterministic softmax maps (..., Kt) on the CPU, as the existing loss tests build them."""
    return torch.softmax(torch.from_numpy(hashrand.normalish(shape, seed)) * sharp, -1)


def misaligned_copy(A):
    """The same values one float into a larger buffer: 4 bytes off every 16-byte boundary."""
    buf = torch.empty(A.numel() + 4, dtype=A.dtype, device=A.device)
    view = buf[1:1 + A.numel()].view(A.shape)
    view.copy_(A)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def hyper_of(over):
    return dict(oloss.DEFAULT_HYPER, **over)


def plans_of(ops, entries, over=None, avg=False):
    """-> (ops.LossPlan, oracle TokenPlan) of one layout."""
    over = over or {}
    return (ops.LossPlan(entries, hyper_of(over), True, .5, 3, avg), oloss.TokenPlan(entries, over, avg))


def reference(A, oplan, last):
    """float64 closed form on the map the kernels read: A (npix, Kt) f32 on the device -> (terms dict, dA (npix, Kt))."""
    npix, Kt = A.shape
    res = int(round(npix ** .5))
    terms, dA = oloss.loss_and_grad_numpy(A.double().cpu().numpy().reshape(res, res, Kt), oplan, smooth=True, sigma=.5,
                                          kernel_size=3, normalize_eot=True, n_prompt_tokens=last + 1)
    return terms, dA.reshape(npix, Kt)


def forward_errors(terms, loss, ref):
    """-> (relative loss error, worst term error in units of its bound) and the assertions of the forward."""
    t = terms.double().cpu().numpy()
    e_loss = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
    worst = 0.0
    for col, key in enumerate(TERM_KEYS):
        want = np.asarray(ref[key], np.float64)
        worst = max(worst, float((np.abs(t[:, col] - want) / (ATOL + RTOL * np.abs(want))).max()))
    return e_loss, worst


def check_forward(terms, loss, ref, what):
    e_loss, worst = forward_errors(terms, loss, ref)
    t = terms.double().cpu().numpy()
    for col, key in enumerate(TERM_KEYS):
        np.testing.assert_allclose(t[:, col], np.asarray(ref[key], np.float64), rtol=RTOL, atol=ATOL, err_msg=f"{what}: {key}")
    np.testing.assert_allclose(float(loss), ref["loss"], rtol=RTOL, err_msg=f"{what}: loss")
    return e_loss, worst


def grad_error(dA, ref):
    ref = torch.as_tensor(ref, dtype=torch.float64)
    return float((dA.double().cpu() - ref).abs().max() / ref.abs().max())


def check_bcast(dPb, dA, dt, what):
    """dP_bcast = dA * SCALE: exactly in f32, within the format's rounding in f16 / bf16."""
    want = dA * SCALE
    if dt == "f32":
        assert torch.equal(dPb, want), what
    else:
        err = float((dPb.float() - want).abs().max() / want.abs().max())
        assert err <= TOL[dt], f"{what}: broadcast map {err:.2e} > {TOL[dt]:.1e}"


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


# --------------------------------------------------------------------------------------- (a) the solo kernels against float64
def test_declared_plans_cover_every_reachable_class(ops):
    assert_coverage(sweep_plans(ops.load()))


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("case", SOLO_CASES, ids=lambda c: c["name"])
def test_solo_kernels_vs_float64(ops, case, dt):
    """ops.aggregate_loss_fwd, ops.smooth_loss_fwd and ops.smooth_loss_bwd under the case's plans: the seven term columns, the
    loss and dA against the float64 closed form evaluated on the very map the kernels read (the f32 average the fused launch
    wrote, itself checked against the float64 average of the head-maps), dP_bcast against dA * scale.

    Measured on the MI355X (worst over the cases and the three head-map types; the bounds are 5e-5 / 1 / 5e-5): see the
    "Loss kernels: LDS plans" section of DESIGN.md."""
    res, Kt, T, last = case["res"], case["Kt"], case["T"], case["last"]
    npix = res * res
    plan, oplan = plans_of(ops, entries_of(T), {"strict": True} if case["strict"] else {}, case["avg"])
    kw = dict(res=res, Kt=Kt, slots=T, strict=case["strict"])
    heads = (1, 2)
    maps = [softmax_maps((h, npix, Kt), 1000 + 7 * res + T + i, case["sharp"]).to("cuda", DT[dt]) for i, h in enumerate(heads)]
    # the fused aggregate + loss forward (its A is a fresh, aligned buffer)
    agg_plan = case["fwd"] if not case["misaligned"] else None
    if agg_plan:
        expect_plan(ops, case["name"], AGG_FWD, agg_plan, **kw)
    A, terms_a, loss_a = ops.aggregate_loss_fwd(maps, res, 1, last, plan)
    mean = torch.cat([m.double() for m in maps]).mean(0)
    e_A = float((A.double() - mean).abs().max() / mean.abs().max())
    assert e_A <= 1e-6, f"A: {e_A:.2e}"
    ref, dA_ref = reference(A, oplan, last)
    A_in = misaligned_copy(A) if case["misaligned"] else A
    pkw = dict(kw, A=A_in)
    expect_plan(ops, case["name"], FWD, case["fwd"], **pkw)
    expect_plan(ops, case["name"], BWD, case["bwd"], **pkw)
    terms, loss = ops.smooth_loss_fwd(A_in, res, 1, last, plan)
    dA, dPb = ops.smooth_loss_bwd(A_in, res, 1, last, plan, None, DT[dt], SCALE)
    ea = forward_errors(terms_a, loss_a.item(), ref)
    es = forward_errors(terms, loss.item(), ref)
    e_grad = grad_error(dA, dA_ref)
    print(f"\n[measured] solo {case['name']} {dt}: fwd {case['fwd']} bwd {case['bwd']} | aggregate_loss_fwd loss {ea[0]:.2e} "
          f"terms {ea[1]:.2f} of the bound | smooth_loss_fwd loss {es[0]:.2e} terms {es[1]:.2f} | smooth_loss_bwd dA {e_grad:.2e}")
    check_forward(terms_a, loss_a.item(), ref, "aggregate_loss_fwd")
    check_forward(terms, loss.item(), ref, "smooth_loss_fwd")
    assert e_grad <= GRAD_TOL, f"dA: {e_grad:.2e} of the gradient's maximum > {GRAD_TOL:.0e}"
    check_bcast(dPb, dA, dt, case["name"])
    assert ops.tickets_are_zero()


# ------------------------------------------------------------------------------------- (b) plans do not change the bits
@pytest.mark.parametrize("case", [c for c in SOLO_CASES if c["misaligned"]], ids=lambda c: c["name"])
def test_misaligned_map_gives_the_same_bits(ops, case):
    """Each pixel row is reduced by one thread in token order whether it is walked in LDS or in global memory: a map that is
    staged (aligned) and its copy that is not (misaligned) give the same terms, loss, dA and dP_bcast, bit for bit."""
    res, Kt, T, last = case["res"], case["Kt"], case["T"], case["last"]
    plan, _ = plans_of(ops, entries_of(T))
    A = softmax_maps((res * res, Kt), 300 + res).cuda()
    B = misaligned_copy(A)
    kw = dict(res=res, Kt=Kt, slots=T)
    for kind in ("fwd", "bwd"):
        staged, unstaged = ops.loss_lds_plan(kind, A=A, **kw), ops.loss_lds_plan(kind, A=B, **kw)
        assert staged.stage_rows >= 64 and unstaged.stage_rows == 0 and staged.use_gcol == unstaged.use_gcol
    expect_plan(ops, case["name"], FWD, case["fwd"], A=B, **kw)
    expect_plan(ops, case["name"], BWD, case["bwd"], A=B, **kw)
    dloss = torch.tensor([1.75], device="cuda")
    for dt in sorted(DT):
        outs = []
        for M in (A, B):
            terms, loss = ops.smooth_loss_fwd(M, res, 1, last, plan)
            dA, dPb = ops.smooth_loss_bwd(M, res, 1, last, plan, dloss, DT[dt], SCALE)
            outs.append((terms, loss, dA, dPb))
        for name, a, b in zip(("terms", "loss", "dA", "dPb"), *outs):
            same_bits(a, b, f"{case['name']} {dt} {name}")
        assert outs[0][2].any()


def _table_plans(ops):
    return [plans_of(ops, e, h, avg)[0] for e, h, _, avg in TABLE_ROWS]


def _image_maps(S, res, Kt, heads, dtype, seed, sharp=3.0):
    """Head-maps of S images, image-major: [(S * h, npix, Kt)] on the device."""
    return [softmax_maps((S * h, res * res, Kt), seed + i, sharp).to("cuda", dtype) for i, h in enumerate(heads)]


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("res", sorted(TABLE_CASES))
def test_table_capacity_does_not_change_the_bits(ops, res, dt):
    """One set of image rows (a strict row, a T = 0 row, an early slice end, an image with dloss = 0) through ImageTables of
    growing capacity T_max: the backward plans go from resident columns and 256 staged rows down to nothing staged, and every
    image keeps its bits — against the smallest capacity and against the solo entry points on its own row."""
    S, heads = len(TABLE_ROWS), (1, 2)
    plans = _table_plans(ops)
    slices = [(1, r[2]) for r in TABLE_ROWS]
    maps = _image_maps(S, res, 77, heads, DT[dt], 50 + res)
    dloss = torch.tensor(TABLE_DLOSS, device="cuda")
    runs = []
    for T_max, fwd, bwd in TABLE_CASES[res]:
        kw = dict(res=res, Kt=77, slots=T_max, images=S, table=True)
        expect_plan(ops, f"table r{res} T_max {T_max}", AGG_FWD, fwd, **kw)
        expect_plan(ops, f"table r{res} T_max {T_max}", BWD, bwd, **kw)
        table = ops.ImageTable(S, T_max, res, True, .5, 3, torch.device("cuda")).set(plans, slices)
        A, terms, loss = ops.aggregate_loss_fwd_images(maps, table)
        dA, dPb = ops.smooth_loss_bwd_images(A, table, dloss, bcast_dtype=DT[dt], bcast_scale=SCALE)
        runs.append((T_max, A, terms, loss, dA, dPb))
    assert ops.tickets_are_zero()
    T0, A0, terms0, loss0, dA0, dPb0 = runs[0]
    for T_max, A, terms, loss, dA, dPb in runs[1:]:
        what = f"r{res} {dt} T_max {T_max} against {T0}"
        same_bits(A, A0, what + " A")
        same_bits(terms[:, :T0], terms0, what + " terms")
        assert not terms[:, T0:].any(), what
        same_bits(loss, loss0, what + " loss")
        same_bits(dA, dA0, what + " dA")
        same_bits(dPb, dPb0, what + " dPb")
    for s, (plan, row) in enumerate(zip(plans, TABLE_ROWS)):      # the smallest capacity against the solo entry points
        if plan.T == 0:
            assert loss0[s].item() == 0 and not terms0[s].any() and not dA0[s].any() and not dPb0[s].any()
            continue
        own = [m.reshape(S, -1, *m.shape[1:])[s] for m in maps]
        A1, t1, l1 = ops.aggregate_loss_fwd(own, res, 1, row[2], plan)
        same_bits(A0[s], A1, f"image {s} A")
        same_bits(terms0[s, :plan.T], t1, f"image {s} terms")
        same_bits(loss0[s:s + 1], l1, f"image {s} loss")
        assert not terms0[s, plan.T:].any()
        if TABLE_DLOSS[s] == 0:
            assert not dA0[s].any() and not dPb0[s].any() and not torch.signbit(dA0[s]).any()
            continue
        d1, p1 = ops.smooth_loss_bwd(A1, res, 1, row[2], plan, dloss[s:s + 1], bcast_dtype=DT[dt], bcast_scale=SCALE)
        same_bits(dA0[s], d1, f"image {s} dA")
        same_bits(dPb0[s], p1, f"image {s} dPb")
        assert d1.any()


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("case", BATCHED_CASES, ids=lambda c: f"T{c[0]}")
def test_batched_launches_keep_the_bits_of_the_solo_ones(ops, case, dt):
    """ga_aggregate_loss_fwd_batched / ga_smooth_loss_bwd_batched at res 32 under plans without resident columns: per image the
    bits of the solo entry points, an image with dloss = 0 exact zeros, and the backward on a misaligned copy of the batched A
    (nothing staged) the same bits again."""
    T, fwd, bwd, bwd_mis = case
    S, res, heads = 3, 32, (1, 2)
    plan, _ = plans_of(ops, entries_of(T))
    kw = dict(res=res, Kt=77, slots=T, images=S)
    expect_plan(ops, f"batched T {T}", AGG_FWD, fwd, **kw)
    maps = _image_maps(S, res, 77, heads, DT[dt], 90 + T)
    A, terms, loss = ops.aggregate_loss_fwd_batched(maps, S, res, 1, 76, plan)
    B = misaligned_copy(A)
    expect_plan(ops, f"batched T {T}", BWD, bwd, A=A, **kw)
    expect_plan(ops, f"batched T {T} misaligned", BWD, bwd_mis, A=B, **kw)
    dloss = torch.tensor([1.5, 0.0, 2.5], device="cuda")
    dA, dPb = ops.smooth_loss_bwd_batched(A, res, 1, 76, plan, dloss, bcast_dtype=DT[dt], bcast_scale=SCALE)
    dA2, dPb2 = ops.smooth_loss_bwd_batched(B, res, 1, 76, plan, dloss, bcast_dtype=DT[dt], bcast_scale=SCALE)
    same_bits(dA2, dA, "misaligned dA")
    same_bits(dPb2, dPb, "misaligned dPb")
    for s in range(S):
        own = [m.reshape(S, -1, *m.shape[1:])[s] for m in maps]
        A1, t1, l1 = ops.aggregate_loss_fwd(own, res, 1, 76, plan)
        same_bits(A[s], A1, f"image {s} A")
        same_bits(terms[s], t1, f"image {s} terms")
        same_bits(loss[s:s + 1], l1, f"image {s} loss")
        if dloss[s] == 0:
            assert not dA[s].any() and not dPb[s].any() and not torch.signbit(dA[s]).any()
            continue
        d1, p1 = ops.smooth_loss_bwd(A1, res, 1, 76, plan, dloss[s:s + 1], bcast_dtype=DT[dt], bcast_scale=SCALE)
        same_bits(dA[s], d1, f"image {s} dA")
        same_bits(dPb[s], p1, f"image {s} dPb")
        assert d1.any()
    assert ops.tickets_are_zero()


@pytest.mark.parametrize("res", sorted(REL_CASES))
def test_relation_capacity_does_not_change_the_bits(ops, res):
    """The relation launches with one fixed set of rows (guided tokens and two relations, no relation, relations alone) through
    tables of Q_max 4, 8 and 16: at res 32 the backward goes from 256 staged rows to 64, the forward drops the resident
    columns — every output keeps its bits."""
    import test_relation_loss_gpu as rel
    rows = [(REL_ENTRIES, 76, REL_RELATIONS), (REL_ENTRIES, 76, None), ([], 40, REL_RELATIONS)]
    A = softmax_maps((3, res, res, 77), 600 + res)
    dloss = torch.tensor([1.25, 1.0, 2.0], device="cuda")
    runs = []
    for Q, fwd, bwd in REL_CASES[res]:
        kw = dict(res=res, Kt=77, slots=4, images=3, table=True, Q_max=Q)
        expect_plan(ops, f"relation r{res} Q_max {Q}", AGG_FWD, fwd, **kw)
        expect_plan(ops, f"relation r{res} Q_max {Q}", BWD, bwd, **kw)
        runs.append(rel._evaluate(rel._table(rows, res, T_max=4, Q_max=Q), A, dloss))
    first = runs[0]
    assert first["rel"][0] > 0 and first["rel"][2] > 0 and first["rel"][1] == 0      # open hinges: the relations reach dA
    assert first["dA"][0].any() and first["dA"][2].any()
    for (Q, _, _), out in zip(REL_CASES[res][1:], runs[1:]):
        for k in ("terms", "box", "rel_terms", "rel", "dA", "dPb"):
            same_bits(out[k], first[k], f"r{res} Q_max {Q} {k}")


def test_relation_small_map_without_resident_columns(ops):
    """One image of 15 x 15 pixels: a relation table of 24 + 16 slots runs its backward without resident columns on a map that
    is staged whole (228 rows).  The bits of the 4 + 4 table, and float64 (the plugin path, as above)."""
    import test_relation_loss_gpu as rel
    res = REL_SMALL_RES
    rows = [(REL_ENTRIES, 76, REL_RELATIONS)]
    A = softmax_maps((1, res, res, 77), 640)
    runs = []
    for T_max, Q, fwd, bwd in REL_SMALL_CASES:
        kw = dict(res=res, Kt=77, slots=T_max, images=1, table=True, Q_max=Q)
        expect_plan(ops, f"relation r15 T_max {T_max} Q_max {Q}", AGG_FWD, fwd, **kw)
        expect_plan(ops, f"relation r15 T_max {T_max} Q_max {Q}", BWD, bwd, **kw)
        runs.append(rel._evaluate(rel._table(rows, res, T_max=T_max, Q_max=Q), A))
    small, large = runs
    T0 = REL_SMALL_CASES[0][0]
    same_bits(large["terms"][:, :T0], small["terms"], "terms")
    assert not large["terms"][:, T0:].any()
    for k in ("box", "rel_terms", "rel", "dA", "dPb"):
        same_bits(large[k], small[k], k)
    l64, g64 = rel._plugin_total(A[0], REL_ENTRIES, 76, REL_RELATIONS, torch.float64, "cpu")
    total = float(large["box"][0].double() + large["rel"][0].double())
    e_loss, e_grad = abs(total - float(l64)) / abs(float(l64)), grad_error(large["dA"][0], g64)
    print(f"\n[measured] relation r15: loss {e_loss:.2e} dA {e_grad:.2e} rel {large['rel'][0].item():.6f}")
    assert large["rel"][0] > 0 and e_loss <= RTOL and e_grad <= GRAD_TOL


# -------------------------------------------------- (c) table, batched and relation forms against float64 away from (1, 256)
FP64_ROWS = [(entries_of(12), {}, 76, False),
             ([_box(3, (.1, .2, .5, .6), "cat"), _coor(7, (.3, .7), "ball"), _box(9, (.4, .3, .5, .5), "cat")],
              {"strict": True, "shrink_factor": .1}, 76, False),
             (entries_of(8), {"shrink_factor": .05}, 40, True)]


@pytest.mark.parametrize("dt", sorted(DT))
def test_table_form_vs_float64_at_res32(ops, dt):
    """ga_aggregate_loss_fwd_images / ga_smooth_loss_bwd_images, S = 3 at res 32 with a table of 16 tokens (an SDXL call with 9
    to 16 guided tokens): forward (0, 256), backward (0, 128).  Per image against the float64 closed form."""
    S, res, (T_max, _, fwd, bwd) = 3, 32, FP64_FORMS["table"]
    kw = dict(res=res, Kt=77, slots=T_max, images=S, table=True)
    expect_plan(ops, "fp64 table", AGG_FWD, fwd, **kw)
    expect_plan(ops, "fp64 table", BWD, bwd, **kw)
    pairs = [plans_of(ops, e, h, avg) for e, h, _, avg in FP64_ROWS]
    assert ops.image_table_capacity(max(p.T for p, _ in pairs)) == T_max
    table = ops.ImageTable(S, T_max, res, True, .5, 3, torch.device("cuda")).set([p for p, _ in pairs],
                                                                                [(1, r[2]) for r in FP64_ROWS])
    maps = _image_maps(S, res, 77, (1, 2), DT[dt], 700)
    A, terms, loss = ops.aggregate_loss_fwd_images(maps, table)
    dA, dPb = ops.smooth_loss_bwd_images(A, table, torch.ones(S, device="cuda"), bcast_dtype=DT[dt], bcast_scale=SCALE)
    for s, ((plan, oplan), row) in enumerate(zip(pairs, FP64_ROWS)):
        ref, dA_ref = reference(A[s], oplan, row[2])
        e_loss, worst = forward_errors(terms[s, :plan.T], loss[s].item(), ref)
        e_grad = grad_error(dA[s], dA_ref)
        print(f"\n[measured] table form {dt} image {s}: loss {e_loss:.2e} terms {worst:.2f} of the bound dA {e_grad:.2e}")
        check_forward(terms[s, :plan.T], loss[s].item(), ref, f"image {s}")
        assert not terms[s, plan.T:].any()
        assert e_grad <= GRAD_TOL, f"image {s} dA: {e_grad:.2e}"
    check_bcast(dPb, dA, dt, "table form")
    assert ops.tickets_are_zero()


@pytest.mark.parametrize("dt", sorted(DT))
def test_batched_form_vs_float64_at_res32(ops, dt):
    """ga_aggregate_loss_fwd_batched / ga_smooth_loss_bwd_batched, S = 3 at res 32 with 14 guided tokens: backward (0, 128)."""
    S, res, (T, _, fwd, bwd) = 3, 32, FP64_FORMS["batched"]
    kw = dict(res=res, Kt=77, slots=T, images=S)
    expect_plan(ops, "fp64 batched", AGG_FWD, fwd, **kw)
    expect_plan(ops, "fp64 batched", BWD, bwd, **kw)
    plan, oplan = plans_of(ops, entries_of(T))
    maps = _image_maps(S, res, 77, (1, 2), DT[dt], 720)
    A, terms, loss = ops.aggregate_loss_fwd_batched(maps, S, res, 1, 76, plan)
    dA, dPb = ops.smooth_loss_bwd_batched(A, res, 1, 76, plan, torch.ones(S, device="cuda"), bcast_dtype=DT[dt],
                                          bcast_scale=SCALE)
    for s in range(S):
        ref, dA_ref = reference(A[s], oplan, 76)
        e_loss, worst = forward_errors(terms[s], loss[s].item(), ref)
        e_grad = grad_error(dA[s], dA_ref)
        print(f"\n[measured] batched form {dt} image {s}: loss {e_loss:.2e} terms {worst:.2f} of the bound dA {e_grad:.2e}")
        check_forward(terms[s], loss[s].item(), ref, f"image {s}")
        assert e_grad <= GRAD_TOL, f"image {s} dA: {e_grad:.2e}"
    check_bcast(dPb, dA, dt, "batched form")
    assert ops.tickets_are_zero()


@pytest.mark.parametrize("dt", sorted(DT))
def test_relation_form_vs_float64_at_res32(ops, dt):
    """ga_aggregate_loss_rel_fwd_images / ga_smooth_loss_rel_bwd_images, S = 3 at res 32, T_max 16 and Q_max 4: forward (0, 256),
    backward (0, 64).  Image 1 carries two relations: box loss + relations against the float64 plugin path (run.ToLeftOf.calc_loss
    with autograd, the oracle's box loss), as test_relation_loss_and_gradient_vs_float64_plugin does; the other images likewise
    with no relation."""
    import test_relation_loss_gpu as rel
    S, res, (T_max, Q, fwd, bwd) = 3, 32, FP64_FORMS["relation"]
    kw = dict(res=res, Kt=77, slots=T_max, images=S, table=True, Q_max=Q)
    expect_plan(ops, "fp64 relation", AGG_FWD, fwd, **kw)
    expect_plan(ops, "fp64 relation", BWD, bwd, **kw)
    rows = [(entries_of(12), 76, None), (REL_ENTRIES, 76, REL_RELATIONS), (entries_of(5), 40, None)]
    table = rel._table(rows, res, T_max=T_max, Q_max=Q)
    # one head-map per image: its average is the map itself, exactly
    maps = [softmax_maps((S, res * res, 77), 740).to("cuda", DT[dt])]
    A, terms, box, rel_terms, rel_loss = ops.aggregate_loss_rel_fwd_images(maps, table)
    same_bits(A, maps[0].float(), "A")
    dA, dPb = ops.smooth_loss_rel_bwd_images(A, table, torch.ones(S, device="cuda"), bcast_dtype=DT[dt], bcast_scale=SCALE)
    assert rel_loss[1] > 0 and rel_loss[0] == 0 and rel_loss[2] == 0
    for s, (entries, last, rels) in enumerate(rows):
        l64, g64 = rel._plugin_total(A[s].cpu().reshape(res, res, 77), entries, last, rels or [], torch.float64, "cpu")
        total = float(box[s].double() + rel_loss[s].double())
        e_loss, e_grad = abs(total - float(l64)) / abs(float(l64)), grad_error(dA[s], g64)
        print(f"\n[measured] relation form {dt} image {s}: loss {e_loss:.2e} dA {e_grad:.2e} rel {rel_loss[s].item():.6f}")
        assert e_loss <= RTOL, f"image {s} loss: {e_loss:.2e}"
        assert e_grad <= GRAD_TOL, f"image {s} dA: {e_grad:.2e}"
    check_bcast(dPb, dA, dt, "relation form")
    assert ops.tickets_are_zero()


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("res", sorted(RAGGED_CASES))
def test_batched_ragged_maps_stage_nothing(ops, res, dt):
    """S = 3 maps of 5 x 5 and 7 x 7 pixels with Kt = 77: an image's slice of the batched A is not 16-byte aligned, the batched
    launches stage nothing while the solo launches stage the padded map.  Per image: the solo launch's bits, and float64.  Flat
    maps and a slice that reaches the last column (see SOLO_CASES): the staging loop's scalar tail carries weight."""
    S, T, last = 3, 3, 77
    plan_b, plan_s = RAGGED_CASES[res]
    kw = dict(res=res, Kt=77, slots=T)
    for kind in (AGG_FWD, BWD):
        expect_plan(ops, f"ragged r{res}", kind, plan_b, images=S, **kw)
    for kind in (FWD, BWD):
        expect_plan(ops, f"ragged r{res} solo", kind, plan_s, **kw)
    assert (res * res * 77) % 4 != 0
    plan, oplan = plans_of(ops, entries_of(T))
    maps = _image_maps(S, res, 77, (1, 2), DT[dt], 760 + res, FLAT)
    A, terms, loss = ops.aggregate_loss_fwd_batched(maps, S, res, 1, last, plan)
    dloss = torch.ones(S, device="cuda")
    dA, dPb = ops.smooth_loss_bwd_batched(A, res, 1, last, plan, dloss, bcast_dtype=DT[dt], bcast_scale=SCALE)
    for s in range(S):
        A1 = A[s].clone()                                    # a fresh buffer: aligned, staged
        t1, l1 = ops.smooth_loss_fwd(A1, res, 1, last, plan)
        d1, p1 = ops.smooth_loss_bwd(A1, res, 1, last, plan, dloss[s:s + 1], bcast_dtype=DT[dt], bcast_scale=SCALE)
        same_bits(terms[s], t1, f"image {s} terms")
        same_bits(loss[s:s + 1], l1, f"image {s} loss")
        same_bits(dA[s], d1, f"image {s} dA")
        same_bits(dPb[s], p1, f"image {s} dPb")
        ref, dA_ref = reference(A[s], oplan, last)
        e_loss, worst = forward_errors(terms[s], loss[s].item(), ref)
        e_grad = grad_error(dA[s], dA_ref)
        print(f"\n[measured] ragged r{res} {dt} image {s}: loss {e_loss:.2e} terms {worst:.2f} of the bound dA {e_grad:.2e}")
        check_forward(terms[s], loss[s].item(), ref, f"image {s}")
        assert e_grad <= GRAD_TOL, f"image {s} dA: {e_grad:.2e}"
    assert ops.tickets_are_zero()
