"""Several prompts, each with its own guidance state, in one batched call — without a GPU: the call form is accepted up to the
device check, every refusal is raised before any launch and names the prompt, the image-table ABI (struct layout, host
validation of the two entry points), and run.execute with batch_across_states (stand-in generation)."""
import ctypes
import os
import re
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ga_hip.h"


def _cpu_pipe(sdxl=False):
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.text import SyntheticTextEncoder, WordTokenizer
    from guided_attention_amd.unet import UNetConfig
    cfg = UNetConfig.tiny(sample_size=32, cross_attention_dim=48)
    if sdxl:
        cfg.addition_embed_type = "text_time"
    unet = SimpleNamespace(config=cfg, device=torch.device("cpu"), dtype=torch.float32)
    return GuidedAttention(unet, None, None, SyntheticTextEncoder(48), WordTokenizer())


def _state(prompt="a robot", **hp):
    from guided_attention_amd.pipeline_guided_attention import GuidanceState
    from guided_attention_amd.utils import shared_state as state
    cfg = SimpleNamespace(prompt=prompt, custom_loss=None, diagnostic_level=0, token_dict={}, thresholds={0: .05},
                          only_update_on_threshold_steps=True, sub_prompt_avg_within=False)
    return GuidanceState(cfg, dict(state.hyperParameterOverrides, **hp))


def _call(pipe, states=None, n=1, **kw):
    states = states if states is not None else [_state("a robot"), _state("a vase", shrink_factor=.1)]
    args = dict(prompt=[st.config.prompt for st in states], attention_store=None, guidance_states=states,
                num_images_per_prompt=n, generator=[torch.Generator().manual_seed(s) for s in range(len(states) * n)])
    args.update(kw)
    return pipe(**args)


@pytest.fixture
def hp():
    from guided_attention_amd.utils import shared_state as state
    saved = state.curHyperParams, getattr(state, "config", None)
    state.curHyperParams = dict(state.hyperParameterOverrides)
    state.config = SimpleNamespace(custom_loss=None, diagnostic_level=0)
    yield state
    state.curHyperParams, state.config = saved


def test_a_mixed_call_reaches_the_device_check(hp):
    from guided_attention_amd._lib import GaError
    with pytest.raises(GaError, match="GPU only"):
        _call(_cpu_pipe())
    with pytest.raises(GaError, match="GPU only"):   # three prompts x two images, prompt embeddings instead of strings
        states = [_state(f"p{p}") for p in range(3)]
        _call(_cpu_pipe(), states, n=2, prompt=None, prompt_embeds=torch.zeros(3, 77, 48),
              negative_prompt_embeds=torch.zeros(3, 77, 48))


def test_guidance_state_is_exported_next_to_the_pipeline():
    import inspect
    from guided_attention_amd import pipeline_guided_attention as pga
    assert "guidance_states" in inspect.signature(pga.GuidedAttention.__call__).parameters
    assert pga.GuidanceState(config=1, hyper_params={}).config == 1


REFUSED = {"custom": "custom-loss plugins", "paint": "paint-with-words", "side_effects": "reference_side_effects",
           "diagnostic": "diagnostic_level > 0", "unfused": "fused_aggregate_loss = False", "optimizer": "use_optimizer",
           "sdxl": "added conditioning", "no_cfg": "guidance_scale <= 1"}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals_name_the_prompt(hp, what):
    pipe = _cpu_pipe(sdxl=what == "sdxl")
    states = [_state("a robot"), _state("a vase"), _state("a cat")]
    bad = 0 if what in ("side_effects", "unfused", "sdxl", "no_cfg") else 2   # call-level refusals: the first prompt
    kw = {}
    if what == "custom":
        states[2].config.custom_loss = {"toLeftOf": (object(), "(a, b)")}
    elif what == "paint":
        states[2].hyper_params["paint_with_words_stop"] = 10
    elif what == "side_effects":
        pipe.reference_side_effects = True
    elif what == "diagnostic":
        states[2].config.diagnostic_level = 1
    elif what == "unfused":
        pipe.fused_aggregate_loss = False
    elif what == "optimizer":
        states[2].hyper_params["use_optimizer"] = True
    elif what == "no_cfg":
        kw["guidance_scale"] = 1.0
    with pytest.raises(NotImplementedError, match=f"prompt {bad}: .*" + re.escape(REFUSED[what])):
        _call(pipe, states, **kw)


def test_inputs_must_match_the_prompts(hp):
    pipe = _cpu_pipe()
    two = [_state("a robot"), _state("a vase")]
    with pytest.raises(ValueError, match="3 guidance_states for 2 prompts"):
        _call(pipe, two + [_state("x")], prompt=["a robot", "a vase"], generator=[torch.Generator()] * 3)
    with pytest.raises(ValueError, match="1 guidance_states for 2 prompts"):
        _call(pipe, two[:1], prompt=["a robot", "a vase"])
    with pytest.raises(ValueError, match="3 generators for 4 images"):
        _call(pipe, two, n=2, generator=[torch.Generator()] * 3)
    with pytest.raises(ValueError, match="one generator per image"):
        _call(pipe, two, generator=torch.Generator())
    with pytest.raises(ValueError, match="latents hold 3 images"):
        _call(pipe, two, generator=None, latents=torch.zeros(3, 4, 32, 32))
    with pytest.raises(ValueError, match="per-image lists"):
        _call(pipe, two, renoise_noise=[[]])
    with pytest.raises(ValueError, match="negative_prompt"):
        _call(pipe, two, negative_prompt="blurry")
    with pytest.raises(ValueError, match="at most 64 images"):
        _call(pipe, two, n=33, generator=[torch.Generator()] * 66)


def test_a_prompt_list_without_states_keeps_its_refusal(hp):
    with pytest.raises(NotImplementedError, match="list of different prompts"):
        _cpu_pipe()(prompt=["a robot", "a vase"], attention_store=None)


def test_image_table_rows_are_checked_on_the_host():
    """Rows are validated before any upload: more tokens than the capacity, a token outside its slice, a box without a pixel
    centre (ZeroDivisionError naming the image, as _check_boxes raises it)."""
    from guided_attention_amd import ops
    from guided_attention_amd._lib import GaError
    assert [ops.image_table_capacity(t) for t in (0, 1, 4, 5, 9, 32)] == [4, 4, 4, 8, 16, 32]
    with pytest.raises(GaError):
        ops.image_table_capacity(33)
    hp = {"inside_loss_scale": .2, "outside_loss_scale": .2, "shrink_factor": 0.0}
    ok = ops.LossPlan([{"index": 2, "kind": "BOX", "geom": (.6, .3, .4, .55), "subprompt": "a"}], hp)
    tiny = ops.LossPlan([{"index": 2, "kind": "BOX", "geom": (.51, .51, .01, .01), "subprompt": "a"}], hp)
    table = object.__new__(ops.ImageTable)   # the host half only: no device buffer is touched before the rows pass
    table.images, table.T_max, table.res = 2, 4, 16
    with pytest.raises(ZeroDivisionError, match="image 1"):
        ops.ImageTable.set(table, [ok, tiny], [(1, 76), (1, 76)])
    with pytest.raises(GaError, match="image 0: token 2 lies outside"):
        ops.ImageTable.set(table, [ok, ok], [(1, 2), (1, 76)])
    many = ops.LossPlan([{"index": 2 + t, "kind": "COOR", "geom": (.5, .5), "subprompt": "a"} for t in range(5)], hp)
    with pytest.raises(GaError, match="image 1: 5 guided tokens"):
        ops.ImageTable.set(table, [ok, many], [(1, 76), (1, 76)])


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_image_loss_struct_layout_matches_header(tmp_path):
    from guided_attention_amd import _lib
    fields = ["first", "last", "T", "strict", "inside_scale", "outside_scale", "center_weight", "shrink", "tok"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ga_hip.h"', "int main(void) {",
           '  printf("size %zu\\n", sizeof(ga_image_loss_t));',
           '  printf("tokens %d\\n", GA_IMAGE_MAX_TOKENS);']
    src += [f'  printf("{f} %zu\\n", offsetof(ga_image_loss_t, {f}));' for f in fields]
    src += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(HEADER.parent), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_lib.ga_image_loss_t) == 1576
    assert int(out["tokens"]) == _lib.GA_IMAGE_MAX_TOKENS == 32
    for f in fields:
        assert int(out[f]) == getattr(_lib.ga_image_loss_t, f).offset, f


@pytest.fixture(scope="module")
def lib():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_table_entry_points_validate_on_the_host(lib):
    """Fake (never dereferenced) device pointers: every call below must fail in the host checks, before any launch."""
    from guided_attention_amd import _lib
    p = ctypes.c_void_p(0x1000)
    hp = _lib.ga_loss_params_t(sigma=.5, ksize=3, smooth=1)
    maps = (ctypes.c_void_p * 1)(0x1000)
    heads = (ctypes.c_int * 1)(8)

    def fwd(images=2, res=16, table=p, T_max=4, A=p, terms=p, tickets=p):
        return lib.ga_aggregate_loss_fwd_images(maps, heads, 1, images, res, 77, table, T_max, ctypes.byref(hp), A, terms, p,
                                                tickets, _lib.GA_F32, None)

    def bwd(images=2, res=16, table=p, T_max=4, A=p, dloss=p, dA=p):
        return lib.ga_smooth_loss_bwd_images(A, images, res, 77, table, T_max, ctypes.byref(hp), dloss, dA, None, 1.0,
                                             _lib.GA_F32, None)

    for call in (fwd, bwd):
        assert call(table=None) == -1 and call(A=None) == -1
        assert call(images=0) == -2 and call(images=65) == -2
        assert call(T_max=33) == -2 and call(T_max=0) == -2
        assert call(res=64, T_max=8) == -2                  # 8 * 64^2 > 24576
        assert call(res=65, T_max=1) == -2
    assert fwd(terms=None) == -1 and fwd(tickets=None) == -1
    assert bwd(dloss=None) == -1 and bwd(dA=None) == -1


# ------------------------------------------------------------------------------------------ run.execute across states
def _execute_worker(rank, world, port, out_dir, per_pass):
    sys.path.insert(0, str(ROOT))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from PIL import Image
    from guided_attention_amd import parallel, run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.text import WordTokenizer
    from guided_attention_amd.utils import helpers, shared_state as state
    if world > 1:
        parallel.init_distributed("gloo")
    metas = ["a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]", "a [cat:.1,.2,.5,.5] on a [mat:.1,.6,.8,.3]"]
    cfg = RunConfig(meta_prompt=metas[0], seeds=[3, 1, 4, 5, 9], output_path=Path(out_dir), seeds_per_pass=per_pass,
                    batch_across_states=True)
    cfg.stable = SimpleNamespace(device=torch.device("cpu"), tokenizer=WordTokenizer())
    # both states name their meta prompt: overrideConfig leaves config.meta_prompt as the previous job set it otherwise
    iterations = [{"meta_prompt": metas[0]}, {"meta_prompt": metas[1], "thresholds": {0: .3, 2: .6}, "shrink_factor": .1}]
    state.hyperParameterIterations = iterations
    calls = []

    def fake_run_on_prompt(prompt, model, controller, seed, config, **extra):
        seeds = [g.initial_seed() for g in seed] if isinstance(seed, list) else [seed.initial_seed()]
        if "guidance_states" in extra:
            sts = extra["guidance_states"]
            assert extra["num_images_per_prompt"] == 1 and prompt == [st.config.prompt for st in sts]
            hps = [int(st.config.meta_prompt == metas[1]) for st in sts]
            for st, h in zip(sts, hps):   # each snapshot is its job's own state
                assert st.config.thresholds == ({0: .3, 2: .6} if h else state.hyperParameterOverrides["thresholds"])
                assert bool(st.config.token_dict) and st.hyper_params.get("shrink_factor") == (.1 if h else
                                                                                              state.hyperParameterOverrides["shrink_factor"])
        else:
            hps = [int(state.config.meta_prompt == metas[1])]
        calls.append(list(zip(seeds, hps)))
        lat = torch.cat([torch.full((1, 4, 8, 8), float(s) + 0.25 * h) for s, h in zip(seeds, hps)])
        imgs = [Image.fromarray(np.full((16, 16, 3), (s * 7 + h) % 251, np.uint8)) for s, h in zip(seeds, hps)]
        logs = [[f"seed {s} state {h}\n"] for s, h in zip(seeds, hps)]
        if len(seeds) == 1:
            helpers.log(f"seed {seeds[0]} state {hps[0]}")
        return SimpleNamespace(images=imgs, latents=lat, logs=logs)

    run.run_on_prompt = fake_run_on_prompt
    try:
        run.execute(cfg)
    finally:
        state.hyperParameterIterations = [{}]
    jobs = [(s, h) for s in cfg.seeds for h in (0, 1)]
    mine = jobs[rank::world]
    assert [j for c in calls for j in c] == mine                              # the stripe, in job order
    assert [len(c) for c in calls] == [min(per_pass, len(mine) - k) for k in range(0, len(mine), per_pass)]
    if len({h for _, h in mine}) == 2:   # (over two ranks the stripe of two alternating states is one state per rank)
        assert any(len({h for _, h in c}) == 2 for c in calls)                # chunks span states
    folders = {0: Path(out_dir) / "a _robot__6,_3,_4,_55_ and a _blue vase__2,_3,_4,_55_",
               1: Path(out_dir) / "a _cat__1,_2,_5,_5_ on a _mat__1,_6,_8,_3_"}
    for s, h in mine:
        name = helpers.dictToString(dict(state.hyperParameterOverrides, **iterations[h]))
        assert (folders[h] / f"{s}{name}.png").exists(), (s, h)
        assert f"seed {s} state {h}" in (folders[h] / f"{s}{name}.txt").read_text()
        assert not (folders[1 - h] / f"{s}{name}.png").exists()
    if rank == 0:
        res = state.last_results
        assert [float(t[0, 0, 0, 0]) for t in res["latents"]] == [s + 0.25 * h for s, h in jobs]   # job order
        assert [int(np.asarray(im)[0, 0, 0]) for im in res["images"]] == [(s * 7 + h) % 251 for s, h in jobs]
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_execute_batches_across_states_in_one_process(tmp_path, monkeypatch):
    from guided_attention_amd import run
    from guided_attention_amd.utils import shared_state as state
    monkeypatch.setattr(run, "run_on_prompt", run.run_on_prompt)
    monkeypatch.setattr(state, "curHyperParams", state.curHyperParams)
    monkeypatch.setattr(state, "config", getattr(state, "config", None), raising=False)
    for k, v in dict(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="0").items():
        monkeypatch.setenv(k, v)
    _execute_worker(0, 1, 0, str(tmp_path), 3)


def test_execute_batches_across_states_over_two_ranks(tmp_path):
    port = 29600 + os.getpid() % 90
    mp.spawn(_execute_worker, args=(2, port, str(tmp_path), 3), nprocs=2, join=True)


def test_batch_across_states_is_a_cli_flag():
    from guided_attention_amd import run
    cfg = run._parse_cli(["--meta_prompt", "a [robot:.6,.3,.4,.55]", "--batch_across_states", "true", "--seeds_per_pass", "3",
                          "--output_path", "/tmp/ga_ppp"])
    assert cfg.batch_across_states is True and cfg.seeds_per_pass == 3
    assert run._parse_cli(["--meta_prompt", "a", "--output_path", "/tmp/ga_ppp"]).batch_across_states is False
