"""S images per call without a GPU: every request the batched path refuses is refused before any launch, and run.execute
with seeds_per_pass chunks each rank's jobs (stand-in generation)."""
import os
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent


def _cpu_pipe(sdxl=False):
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.text import SyntheticTextEncoder, WordTokenizer
    from guided_attention_amd.unet import UNet2DConditionModel, UNetConfig
    cfg = UNetConfig.tiny(sample_size=32, cross_attention_dim=48)
    if sdxl:
        cfg.addition_embed_type = "text_time"
    unet = SimpleNamespace(config=cfg, device=torch.device("cpu"), dtype=torch.float32)
    return GuidedAttention(unet, None, None, SyntheticTextEncoder(48), WordTokenizer())


def _call(pipe, **kw):
    args = dict(prompt="a robot", attention_store=None, num_images_per_prompt=3,
                generator=[torch.Generator().manual_seed(s) for s in range(3)])
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


def test_batched_call_reaches_the_device_check_when_valid(hp):
    from guided_attention_amd._lib import GaError
    with pytest.raises(GaError, match="GPU only"):
        _call(_cpu_pipe())


REFUSED = {"custom": "custom-loss plugins", "paint": "paint-with-words", "side_effects": "reference_side_effects",
           "diagnostic": "diagnostic_level > 0", "unfused": "fused_aggregate_loss = False", "optimizer": "use_optimizer",
           "sdxl": "added conditioning"}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused_features_raise_before_any_launch(hp, what):
    pipe = _cpu_pipe(sdxl=what == "sdxl")
    if what == "custom":
        hp.config.custom_loss = {"toLeftOf": (object(), "(a, b)")}
    elif what == "paint":
        hp.curHyperParams["paint_with_words_stop"] = 10
    elif what == "side_effects":
        pipe.reference_side_effects = True
    elif what == "diagnostic":
        hp.config.diagnostic_level = 1
    elif what == "unfused":
        pipe.fused_aggregate_loss = False
    elif what == "optimizer":
        hp.curHyperParams["use_optimizer"] = True
    with pytest.raises(NotImplementedError, match=re.escape(REFUSED[what]) + ".*num_images_per_prompt > 1"):
        _call(pipe)


def test_a_list_of_prompts_is_refused(hp):
    with pytest.raises(NotImplementedError, match="list of different prompts"):
        _call(_cpu_pipe(), prompt=["a robot", "a vase"])


def test_inputs_must_be_per_image(hp):
    pipe = _cpu_pipe()
    with pytest.raises(ValueError, match="one generator per image"):
        _call(pipe, generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="2 generators for 3 images"):
        _call(pipe, generator=[torch.Generator(), torch.Generator()])
    with pytest.raises(ValueError, match="latents hold 2 images"):
        _call(pipe, generator=None, latents=torch.zeros(2, 4, 32, 32))
    with pytest.raises(ValueError, match="per-image lists"):
        _call(pipe, renoise_noise=[[], []])
    with pytest.raises(ValueError, match="list of generators or `latents`"):
        _call(pipe, generator=None)


def test_seeds_per_pass_is_a_cli_flag():
    from guided_attention_amd import run
    cfg = run._parse_cli(["--meta_prompt", "a [robot:.6,.3,.4,.55]", "--seeds_per_pass", "4", "--output_path", "/tmp/ga_spp"])
    assert cfg.seeds_per_pass == 4


def test_stored_maps_select_one_image():
    from guided_attention_amd.utils.ptp_utils import stored_maps
    maps = [torch.arange(3 * 2 * 4 * 5, dtype=torch.float32).reshape(6, 4, 5)]
    store = SimpleNamespace(get_average_attention=lambda: {"up_cross": maps, "down_cross": [], "mid_cross": []})
    assert stored_maps(store, 2, ("up", "down", "mid"), True, 0)[0] is maps[0]
    got = stored_maps(store, 2, ("up", "down", "mid"), True, 2, images=3)[0]
    assert torch.equal(got, maps[0].reshape(3, -1, 4, 5)[2])
    with pytest.raises(IndexError):
        stored_maps(store, 2, ("up", "down", "mid"), True, 3, images=3)


# ------------------------------------------------------------------------------------------ run.execute with seeds_per_pass
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
    cfg = RunConfig(meta_prompt="a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]", seeds=[3, 1, 4, 1, 5, 9, 2],
                    output_path=Path(out_dir), seeds_per_pass=per_pass)
    cfg.stable = SimpleNamespace(device=torch.device("cpu"), tokenizer=WordTokenizer())
    state.hyperParameterIterations = [{}, {"inside_loss_scale": .3}]   # two states per seed -> 14 jobs
    calls = []

    def fake_run_on_prompt(prompt, model, controller, seed, config, **extra):
        hp = 0 if state.curHyperParams["inside_loss_scale"] == .2 else 1
        seeds = [g.initial_seed() for g in seed] if isinstance(seed, list) else [seed.initial_seed()]
        calls.append((seeds, hp, extra.get("num_images_per_prompt", 1)))
        lat = torch.cat([torch.full((1, 4, 8, 8), float(s) + 0.25 * hp) for s in seeds])
        imgs = [Image.fromarray(np.full((16, 16, 3), (s * 7 + hp) % 251, np.uint8)) for s in seeds]
        logs = [[f"seed {s} state {hp}\n"] for s in seeds]
        if len(seeds) == 1:
            helpers.log(f"seed {seeds[0]} state {hp}")
        return SimpleNamespace(images=imgs, latents=lat, logs=logs)

    run.run_on_prompt = fake_run_on_prompt
    try:
        run.execute(cfg)
    finally:
        state.hyperParameterIterations = [{}]
    jobs = [(s, h) for s in cfg.seeds for h in (0, 1)]
    mine = jobs[rank::world]
    flat = [(s, h) for seeds, h, _ in calls for s in seeds]
    assert flat == mine                                                      # the stripe, in order
    for seeds, h, n in calls:                                                # chunks: one state, at most per_pass
        assert n == len(seeds) <= per_pass
    expect, cur = [], []
    for s, h in mine:                                                        # consecutive jobs of one state, greedily
        if cur and (len(cur) == per_pass or cur[-1][1] != h):
            expect.append(cur)
            cur = []
        cur.append((s, h))
    expect.append(cur)
    assert [[(s, h) for s in seeds] for seeds, h, _ in calls] == expect
    folder = Path(out_dir) / "a _robot__6,_3,_4,_55_ and a _blue vase__2,_3,_4,_55_"
    for s, h in mine:
        name = helpers.dictToString(dict(state.hyperParameterOverrides, **({"inside_loss_scale": .3} if h else {})))
        assert (folder / f"{s}{name}.png").exists()
        assert f"seed {s} state {h}" in (folder / f"{s}{name}.txt").read_text()
    if rank == 0:
        res = state.last_results
        assert [float(t[0, 0, 0, 0]) for t in res["latents"]] == [s + 0.25 * h for s, h in jobs]   # job order
        assert [int(np.asarray(im)[0, 0, 0]) for im in res["images"]] == [(s * 7 + h) % 251 for s, h in jobs]
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("per_pass", [1, 2, 3])
def test_execute_chunks_jobs_in_one_process(tmp_path, monkeypatch, per_pass):
    from guided_attention_amd import run
    monkeypatch.setattr(run, "run_on_prompt", run.run_on_prompt)
    for k, v in dict(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="0").items():
        monkeypatch.setenv(k, v)
    _execute_worker(0, 1, 0, str(tmp_path), per_pass)


def test_execute_stripes_then_chunks_over_two_ranks(tmp_path):
    port = 29700 + os.getpid() % 90
    mp.spawn(_execute_worker, args=(2, port, str(tmp_path), 2), nprocs=2, join=True)
