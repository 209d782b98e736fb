"""SGD-momentum refinement (`use_optimizer`) without a GPU: the new entry point is declared, bound, exported and validates its
arguments on the host; run.execute keeps jobs of a `use_optimizer` state out of batched calls; the reference fixture holds the
branch the issue describes."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, load_json, load_npz

HEADER = ROOT / "include" / "ga_hip.h"


@pytest.fixture(scope="module")
def lib():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entry_is_declared_bound_and_wrapped():
    from guided_attention_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint ga_latent_sgd_momentum\s*\(", text)
    assert len(_lib.PROTOTYPES["ga_latent_sgd_momentum"]) == 10
    assert int(re.search(r"#define GA_VERSION (\d+)", text).group(1)) == _lib.GA_VERSION
    with pytest.raises(ops.GaError, match="GPU only"):
        ops.latent_sgd_momentum(torch.zeros(4), torch.zeros(4), torch.zeros(4), 1.0, 0.8, True)


def test_loader_names_an_export_the_library_lacks(lib, monkeypatch):
    """ga_latent_sgd_momentum was added under an unchanged GA_VERSION (a pure addition), so the version check cannot tell a
    library built before it from one built after: the loader reports the missing symbol by name instead."""
    from guided_attention_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "PROTOTYPES", dict(_lib.PROTOTYPES, ga_not_in_this_build=[]))
    with pytest.raises(_lib.GaError, match="does not export ga_not_in_this_build"):
        _lib.load()


def test_entry_validates_on_the_host(lib):
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below returns before a launch
    f = lib.ga_latent_sgd_momentum
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        x, g, m, out = args
        assert f(x, g, m, 1.0, 0.8, 1, out, 16, 0, None) == -1
    assert f(p, p, p, 1.0, 0.8, 1, p, 0, 0, None) == -2          # n = 0
    assert f(p, p, p, 1.0, 0.8, 1, p, -5, 0, None) == -2
    assert f(p, p, p, 1.0, 1.0, 1, p, 16, 0, None) == -2         # mu outside [0, 1)
    assert f(p, p, p, 1.0, -0.1, 0, p, 16, 0, None) == -2
    assert f(p, p, p, 1.0, float("nan"), 0, p, 16, 0, None) == -2
    assert f(p, p, p, 1.0, 0.8, 1, p, 16, 3, None) == -3         # unknown dtype
    assert f(p, p, p, 1.0, 0.8, 1, p, 16, -1, None) == -3


def test_fixture_holds_the_momentum_branch_of_the_reference():
    """tests/golden/g12_momentum.*: the reference's own `__call__` with use_optimizer (make_golden_momentum.py).  The g9 case takes
    20 optimizer steps in two refinement calls that both run into the cap, logs `gradient size average` only for the two plain
    updates of the caller, and ends somewhere else than the plain run of g9 (different arithmetic, not noise)."""
    meta = {m["name"]: m for m in load_json("g12_momentum.json")}
    g9 = {m["name"]: m for m in load_json("g9_loop.json")}["no_recurse_thr2"]
    m = meta["momentum_g9"]
    assert m["hyper"]["use_optimizer"] is True and m["thresholds"] == g9["thresholds"] and m["unet_seed"] == g9["unet_seed"]
    assert (m["fwd_b1"], m["fwd_b2"], m["subiterations"], m["bwd"], m["optimizer_steps"]) == (27, 5, 20, 2, 20)
    assert (g9["fwd_b1"], g9["fwd_b2"], g9["subiterations"], g9["bwd"]) == (27, 5, 20, 22)
    g = load_npz("g12_momentum.npz")
    np.testing.assert_allclose(g["momentum_g9.refine_final_losses"], [1.4871, 2.0140], atol=5e-5)
    assert abs(m["final_abs_mean"] - 6.19198) < 1e-5
    ref, plain = g["momentum_g9.final_latents"], load_npz("g9_loop.npz")["no_recurse_thr2.final_latents"]
    assert np.abs(ref - plain).max() / np.abs(plain).max() > 0.1
    w = meta["momentum_wide"]
    assert w["steps"] == 3 and w["optimizer_steps"] == 20 and w["bwd"] == 2 and w["plain"]["bwd"] == 22
    assert g["momentum_wide.final_latents"].shape == g["momentum_wide.plain_final_latents"].shape == (1, 4, 32, 32)
    for case in (m, w, w["plain"]):        # every branch decision of the generating run was at least 5 % clear of its threshold
        assert case["min_margin"] >= 0.05


# ------------------------------------------------------------------------------------------ run.execute
def _sweep(tmp_path, monkeypatch, iterations, seeds, per_pass, across=False):
    """run.execute over `iterations` (hyperParameterIterations) with a stand-in for the generation -> [(seeds, state name, images
    of the call, states of a guidance_states call)] in call order, and the output folder."""
    from PIL import Image
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.text import WordTokenizer
    from guided_attention_amd.utils import helpers, shared_state as state
    for k, v in dict(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0").items():
        monkeypatch.setenv(k, v)
    cfg = RunConfig(meta_prompt="a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]", seeds=list(seeds),
                    output_path=Path(tmp_path), seeds_per_pass=per_pass)
    cfg.batch_across_states = across
    cfg.stable = SimpleNamespace(device=torch.device("cpu"), tokenizer=WordTokenizer())
    monkeypatch.setattr(state, "hyperParameterIterations", iterations)
    calls = []

    def fake_run_on_prompt(prompt, model, controller, seed, config, **extra):
        gens = seed if isinstance(seed, list) else [seed]
        seeds_ = [g.initial_seed() for g in gens]
        states = extra.get("guidance_states")
        n = extra.get("num_images_per_prompt", 1) * (len(states) if states else 1)
        assert n == len(seeds_)
        optimizer = [bool(s.hyper_params.get("use_optimizer")) for s in states] if states else \
            [bool(state.curHyperParams.get("use_optimizer"))] * n
        calls.append((seeds_, optimizer))
        if len(seeds_) == 1:
            helpers.log(f"seed {seeds_[0]} optimizer {optimizer[0]}")
        return SimpleNamespace(images=[Image.fromarray(np.full((16, 16, 3), s % 251, np.uint8)) for s in seeds_],
                               latents=torch.cat([torch.full((1, 4, 8, 8), float(s)) for s in seeds_]),
                               logs=[[f"seed {s} optimizer {o}\n"] for s, o in zip(seeds_, optimizer)])

    monkeypatch.setattr(run, "run_on_prompt", fake_run_on_prompt)
    run.execute(cfg)
    folder = Path(tmp_path) / "a _robot__6,_3,_4,_55_ and a _blue vase__2,_3,_4,_55_"
    return calls, folder


def test_execute_runs_a_use_optimizer_state_as_solo_calls(tmp_path, monkeypatch):
    """seeds_per_pass = 2 over one state: the plain state is guided two seeds per call, the `use_optimizer` state one seed per
    call (the batched call refuses it: before this, the chunk [3, 1] reached that refusal)."""
    plain, _ = _sweep(tmp_path / "p", monkeypatch, [{}], [3, 1, 4], 2)
    assert plain == [([3, 1], [False, False]), ([4], [False])]
    calls, folder = _sweep(tmp_path / "m", monkeypatch, [{"use_optimizer": True}], [3, 1, 4], 2)
    assert calls == [([3], [True]), ([1], [True]), ([4], [True])]
    names = sorted(p.name for p in folder.glob("*.txt"))
    assert len(names) == 3 and all("use_optimizer_True" in n for n in names)
    for s in (3, 1, 4):
        (txt,) = [p for p in folder.glob(f"{s}_*.txt")]
        assert f"seed {s} optimizer True" in txt.read_text()


def test_execute_sweep_over_plain_and_use_optimizer_states(tmp_path, monkeypatch):
    """The sweep {plain, use_optimizer} x seeds with seeds_per_pass = 2.  In one process the jobs of a seed are consecutive
    (job order is seed-major), so chunks that hold two jobs need batch_across_states; a third, plain state makes such chunks
    possible next to the momentum state: the two plain states of a seed share a batched call (guidance_states), the momentum
    state of that seed is a solo call in between, and no batched call ever holds a `use_optimizer` state."""
    iterations = [{}, {"inside_loss_scale": .3}, {"use_optimizer": True}]
    calls, folder = _sweep(tmp_path, monkeypatch, iterations, [3, 1], 2, across=True)
    assert calls == [([3, 3], [False, False]), ([3], [True]), ([1, 1], [False, False]), ([1], [True])]
    assert len(list(folder.glob("*use_optimizer_True*.png"))) == 2 and len(list(folder.glob("*use_optimizer_False*.png"))) == 4
    # without the third state every chunk would be [plain, momentum] of one seed: all solo now
    calls, _ = _sweep(tmp_path / "two", monkeypatch, [{}, {"use_optimizer": True}], [3, 1], 2, across=True)
    assert calls == [([3], [False]), ([3], [True]), ([1], [False]), ([1], [True])]
