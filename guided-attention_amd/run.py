"""Entry points with the reference's names (run.py): `setup`, `load_model`, `parseMetaPrompt`,
`overrideConfig`, `run_on_prompt`, `execute`, the custom-loss plugin API (`CustomLossBase`,
`register_custom_loss`, `ToLeftOf`) and a `main()` CLI taking the RunConfig fields as `--flags` (argparse:
pyrallis is not available here).  `--interactive true` starts the Flask front-end of gui.py."""
import argparse
import copy
import dataclasses
import sys
from abc import ABC, abstractmethod
from pathlib import Path
from typing import List

import torch

from .config import RunConfig
from .pipeline_guided_attention import GuidanceState, GuidedAttention
from .utils import helpers, ptp_utils, shared_state
from .utils.ptp_utils import AttentionStore


def load_model(config: RunConfig, random_init=None):
    """reference run.py:18-29.  Model ids resolve to local folders only (no network); set
    GA_RANDOM_INIT=1 or pass random_init=True to build seeded random weights of the architecture.
    Under torch.distributed.run (WORLD_SIZE > 1) every rank builds the architecture on its own GPU, only rank 0
    reads / initialises the weights, and ONE bucketed RCCL broadcast over xGMI hands them to the other ranks."""
    import os
    from . import parallel
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the guided-attention path runs on HIP kernels only")
    rank, world, local = parallel.init_distributed()
    device = torch.device("cuda", local if "LOCAL_RANK" in os.environ else 0)
    name = "stabilityai/stable-diffusion-2-1-base" if config.sd_2_1 else "CompVis/stable-diffusion-v1-4"
    name = os.environ.get("GA_MODEL_DIR", name)
    if random_init is None:
        random_init = os.environ.get("GA_RANDOM_INIT", "0") == "1"
    revision = "fp16" if config.half_precision else None
    stable = GuidedAttention.from_pretrained(name, revision=revision, random_init=random_init, weights=(rank == 0))
    stable = stable.to(device)
    if world > 1:
        for module in (stable.unet, stable.vae, stable.text_encoder):
            if isinstance(module, torch.nn.Module):
                parallel.broadcast_module_(module)
    # the UNet passes replay as hipGraphs (captured in the first image's warm-up); GA_EAGER=1 launches every kernel
    # from the host instead (same kernels, same results, ~3x slower at batch 1)
    stable.use_graphs = os.environ.get("GA_EAGER", "0") != "1"
    return stable


def run_on_prompt(prompt: List[str], model: GuidedAttention, controller: AttentionStore, seed: torch.Generator,
                  config: RunConfig, **extra):
    if controller is not None:
        ptp_utils.register_attention_control(model, controller)
    outputs = model(prompt=prompt, attention_store=controller, attention_res=config.attention_res,
                    guidance_scale=config.guidance_scale, generator=seed,
                    num_inference_steps=config.n_inference_steps, max_iter_to_alter=config.max_iter_to_alter,
                    run_standard_sd=config.run_standard_sd, thresholds=config.thresholds,
                    scale_factor=config.scale_factor, scale_range=config.scale_range,
                    smooth_attentions=config.smooth_attentions, sigma=config.sigma, kernel_size=config.kernel_size,
                    sd_2_1=config.sd_2_1, **extra)
    return outputs.images[0] if not extra else outputs


def get_indices(tokenized_prompt, tokens):
    n = len(tokens)
    for i in range(0, len(tokenized_prompt) - n):
        if tokenized_prompt[i:i + n] == tokens:
            return list(range(i, i + n))
    return None  # the reference falls through the same way; parseMetaPrompt then raises TypeError


def overrideConfig(config):
    if "meta_prompt" in shared_state.curHyperParams:
        config.meta_prompt = shared_state.curHyperParams["meta_prompt"]
    if "thresholds" in shared_state.curHyperParams:
        config.thresholds = shared_state.curHyperParams["thresholds"]


def parseMetaPrompt(config):
    config.prompt, config.meta_info, config.custom_loss = helpers.parse_prompt(config.meta_prompt)
    shared_state.config = config
    tok = config.stable.tokenizer
    tokenized_prompt = tok(config.prompt)["input_ids"]
    token_dict = {}
    for phrase, kind, geom in config.meta_info:
        tokens = tok(phrase)["input_ids"][1:-1]
        for idx in get_indices(tokenized_prompt, tokens):
            token_dict[idx] = {"word": tok.decode(tokenized_prompt[idx]), "loss_type": kind, "loss": geom,
                               "subprompt": phrase}
    config.token_dict = token_dict


def execute(config, save=True):
    """One image per (seed, hyper-parameter state) (reference run.py:93-135).  config.seeds_per_pass = S > 1 guides up to S
    consecutive jobs of a rank that share a hyper-parameter state in one batched call (same files, same order); with
    config.batch_across_states the chunks may span states, each job guided by a GuidanceState snapshot of its own
    (config after overrideConfig + parseMetaPrompt, and its hyper-parameters) in a call with guidance_states.  A job whose state sets
    `use_optimizer` (SGD-momentum refinement) runs as a chunk of one unless config.batched_momentum_refinement is set: then the
    ordinary chunking rule holds for it and the batched call serves it per image.  The reference runs them serially on one
    device; images of different (seed, state) are independent, so under torch.distributed.run the job list is striped
    over the ranks (job j on rank j % world, one process per GPU, no per-step exchange) and rank 0 gathers the final
    latents and images back into job order.  Single process: exactly the reference's serial loop.
    Returns the path of the last job's image (as the reference does); on rank 0 `shared_state.last_results` holds
    {"latents": [...], "images": [...]} in job order (None on the other ranks)."""
    from . import parallel
    from .utils import vis_utils
    rank, world = parallel.rank_world()
    jobs = [(seed, hp) for seed in config.seeds for hp in shared_state.get_hyperparam_states()]
    images, latents, image_path, paths = [], [], None, {}
    names, snapshots = {}, {}
    across = bool(getattr(config, "batch_across_states", False))
    for j, (seed, hp) in enumerate(jobs):
        shared_state.curHyperParams = hp
        overrideConfig(config)
        parseMetaPrompt(config)
        names[j] = (config.output_path / helpers.get_inner_folder_name(), helpers.dictToString(shared_state.curHyperParams))
        paths[j] = names[j][0] / f"{seed}{names[j][1]}.png"
        if across:   # parseMetaPrompt assigns fresh prompt / meta_info / token_dict objects: a shallow copy is a snapshot
            snapshots[j] = GuidanceState(copy.copy(config), hp)
    # this rank's jobs (striped as before), run in consecutive chunks of up to seeds_per_pass jobs sharing one
    # hyper-parameter state: one batched call per chunk (num_images_per_prompt = chunk size)
    mine = [j for j in range(len(jobs)) if j % world == rank]
    per_pass = max(int(getattr(config, "seeds_per_pass", 1) or 1), 1)
    chunks = []
    momentum = bool(getattr(config, "batched_momentum_refinement", False))
    # a batched call refuses use_optimizer unless the pipeline is told to serve it: chunks of one
    solo = lambda j: not momentum and bool(jobs[j][1].get("use_optimizer", False))   # noqa: E731
    for j in mine:
        if chunks and len(chunks[-1]) < per_pass and not solo(j) and not solo(chunks[-1][0]) and \
                (across or jobs[chunks[-1][0]][1] == jobs[j][1]):
            chunks[-1].append(j)
        else:
            chunks.append([j])
    for chunk in chunks:
        hp = jobs[chunk[0]][1]
        shared_state.curHyperParams = hp
        overrideConfig(config)
        parseMetaPrompt(config)
        helpers.log_clear()
        seeds = [jobs[j][0] for j in chunk]
        shared_state.cur_seed = seeds[0]
        for seed in seeds:
            print(f"Seed: {seed}")
        controller = AttentionStore()
        config.stable.fused_relation_loss = bool(getattr(config, "fused_relation_loss", False))
        config.stable.own_vae_decode = bool(getattr(config, "own_vae_decode", False))
        if len(chunk) > 1:   # the declared variant: a batched call refuses paint-with-words unless the pipeline is told to serve it
            config.stable.batched_paint_with_words = bool(getattr(config, "batched_paint_with_words", False))
            config.stable.batched_momentum_refinement = momentum
        if len(chunk) == 1:
            g = torch.Generator(config.stable.device).manual_seed(seeds[0])
            out = run_on_prompt(prompt=config.prompt, model=config.stable, controller=controller, seed=g, config=config,
                                output_type="pil")
            results = [(out.images[0], out.latents.detach(), list(helpers.lines))]
        elif across:   # one prompt per job, each with its own state; the call's own `thresholds` is not read in this form
            gens = [torch.Generator(config.stable.device).manual_seed(seed) for seed in seeds]
            out = run_on_prompt(prompt=[snapshots[j].config.prompt for j in chunk], model=config.stable, controller=controller,
                                seed=gens, config=config, output_type="pil", num_images_per_prompt=1,
                                guidance_states=[snapshots[j] for j in chunk])
            results = [(out.images[k], out.latents[k:k + 1].detach(), out.logs[k]) for k in range(len(chunk))]
        else:
            gens = [torch.Generator(config.stable.device).manual_seed(seed) for seed in seeds]
            out = run_on_prompt(prompt=config.prompt, model=config.stable, controller=controller, seed=gens, config=config,
                                output_type="pil", num_images_per_prompt=len(chunk))
            results = [(out.images[k], out.latents[k:k + 1].detach(), out.logs[k]) for k in range(len(chunk))]
        for j, (image, lat, lines) in zip(chunk, results):
            seed = jobs[j][0]
            out_dir, name = names[j]
            if across and jobs[j][1] is not shared_state.curHyperParams:   # the job's own state while its files are written
                shared_state.curHyperParams = jobs[j][1]
                overrideConfig(config)
                parseMetaPrompt(config)
            images.append(image)
            latents.append(lat)
            if save:
                helpers.lines = list(lines)
                out_dir.mkdir(exist_ok=True, parents=True)
                helpers.annotate_image(image)
                try:
                    image.save(paths[j])
                except OSError:
                    print("bad path. this is often due to exceeding max path length.")
                    name = ""
                    paths[j] = out_dir / f"{seed}.png"
                    image.save(paths[j])
                helpers.log_save(out_dir / f"{seed}{name}.txt")
                helpers.save_latent_stats(out_dir / f"{seed}{name}figure.png")
    if jobs and chunks and chunks[-1][-1] != len(jobs) - 1:   # leave the last job's state behind, as the serial loop does
        shared_state.curHyperParams = jobs[-1][1]
        overrideConfig(config)
        parseMetaPrompt(config)
    if jobs:
        image_path = paths[len(jobs) - 1]
    if world > 1:
        import numpy as np
        from PIL import Image
        dev = config.stable.device
        pix = [torch.from_numpy(np.asarray(im.convert("RGB")).copy()).to(dev) for im in images]
        g_lat, g_pix = parallel.gather_tensors(latents), parallel.gather_tensors(pix)
        if rank == 0:
            latents = parallel.unstripe(g_lat)
            images = [Image.fromarray(t.cpu().numpy()) for t in parallel.unstripe(g_pix)]
    shared_state.last_results = {"latents": latents, "images": images} if rank == 0 else None
    if rank == 0 and save and images:
        joined = vis_utils.get_image_grid(images)  # a grid of the results across all seeds (reference :131-134)
        if not config.interactive:
            helpers.annotate_image(joined)
        joined.save(config.output_path / f"{helpers.get_meta_prompt_clean()}.png")
    return image_path


skipLoading = False


def setup(config, random_init=None):
    shared_state.config = config
    if not skipLoading:
        config.stable = load_model(config, random_init=random_init)


class CustomLossBase(ABC):
    """Plugin API of the reference (run.py:148-176): a Python loss over the (H, W, n_text_tokens) map
    softmax(100 * A[:, :, 1:last]); it is added to the fused loss and differentiated by autograd."""

    @abstractmethod
    def calc_loss(self, cross_attention_maps, text_args: str) -> torch.Tensor:
        pass

    def subprompts_of_interest(self, text_args: str) -> list:
        return []

    def parse_text_args(self, text_args: str):
        import ast
        return ast.literal_eval(text_args)

    def find_indices_for_sub_prompt(self, sub_prompt):
        tok = shared_state.config.stable.tokenizer
        full = tok(shared_state.config.prompt)["input_ids"][1:-1]
        sub = tok(sub_prompt)["input_ids"][1:-1]
        for i in range(len(full) - len(sub) + 1):
            if full[i:i + len(sub)] == sub:
                return list(range(i, i + len(sub)))

    def get_map_for_token(self, cross_attention_maps, token_index: int, pixel_wise_normalization=True):
        image_map = cross_attention_maps[:, :, token_index]
        return image_map / image_map.sum() if pixel_wise_normalization else image_map


class DirectionalRelation(CustomLossBase):
    """The arithmetic the four directional relations share (reference run.py:180-225, its ToLeftOf): along one map axis —
    `axis` 1: the column j + .5 with the map width, 0: the row i + .5 with the map height, row 0 on top — the attention
    centroid of the sub-prompt in the "left" role must have a coordinate at least 20 % of that extent smaller than the other one's.  `lead` is the
    position (0: a, 1: b) of the argument in that role: it is added, and its token count divides BOTH centroid sums, as the
    reference normalises.  Plain PyTorch on the GPU map; differentiated by autograd and added to the fused loss."""

    axis = 1
    lead = 0

    def calc_loss(self, cross_attention_maps, text_args: str) -> torch.Tensor:
        args = self.parse_text_args(self.quote_items_in_tuple(text_args))
        left = self.find_indices_for_sub_prompt(args[self.lead])
        right = self.find_indices_for_sub_prompt(args[1 - self.lead])
        width = cross_attention_maps.shape[self.axis]
        cols = torch.arange(width, device=cross_attention_maps.device, dtype=cross_attention_maps.dtype) + 0.5
        coords = cols[None, :] if self.axis == 1 else cols[:, None]

        def centroid(idx):
            total = cross_attention_maps.new_zeros(1)
            for i in idx:
                total = total + (self.get_map_for_token(cross_attention_maps, i, True) * coords).sum() / len(left)
            return total

        gap = .2 * width
        loss = (centroid(left) + gap - centroid(right)) / width * 9
        return torch.clamp(loss, min=0)

    def subprompts_of_interest(self, text_args: str) -> list:
        return list(self.parse_text_args(self.quote_items_in_tuple(text_args)))

    def quote_items_in_tuple(self, text_args):
        items = text_args.strip("()").split(",")
        return "(" + ",".join(f"'{item.strip()}'" for item in items) + ")"


class ToLeftOf(DirectionalRelation):
    """`[CustomLoss:toLeftOf (a, b)]`: the attention centroid of sub-prompt a must sit at least 20 % of the map width
    to the left of b's (reference run.py:180-225, including its normalisation of BOTH centroids by the token count
    of the left sub-prompt)."""


class ToRightOf(DirectionalRelation):
    """`[CustomLoss:toRightOf (a, b)]`: a's centroid at least 20 % of the map width to the right of b's — toLeftOf (b, a)."""
    lead = 1


class Above(DirectionalRelation):
    """`[CustomLoss:above (a, b)]`: a's centroid at least 20 % of the map height above b's (row 0 is the top row) — toLeftOf on
    the spatially transposed map."""
    axis = 0


class Below(DirectionalRelation):
    """`[CustomLoss:below (a, b)]`: a's centroid at least 20 % of the map height below b's — above (b, a)."""
    axis = 0
    lead = 1


BUILTIN_LOSSES = {"toLeftOf": ToLeftOf, "toRightOf": ToRightOf, "above": Above, "below": Below}


def register_custom_loss(name: str, customLoss: CustomLossBase):
    if not hasattr(shared_state.config, "registered_loss_functions"):
        shared_state.config.registered_loss_functions = {}
    shared_state.config.registered_loss_functions[name] = customLoss


def register_builtin_losses():
    """Registers the four directional relations under their prompt names: toLeftOf, toRightOf, above, below."""
    for name, cls in BUILTIN_LOSSES.items():
        register_custom_loss(name, cls())


def _parse_cli(argv):
    ap = argparse.ArgumentParser(description="guided-attention sampling on MI355X")
    for f in dataclasses.fields(RunConfig):
        flag = f"--{f.name}"
        if f.type is bool or isinstance(f.default, bool):
            ap.add_argument(flag, type=lambda s: s.lower() in ("1", "true", "yes"), default=f.default)
        elif f.name == "seeds":
            ap.add_argument(flag, type=lambda s: [int(x) for x in s.strip("[]").split(",")], default=[42])
        elif f.name == "thresholds":
            ap.add_argument(flag, type=lambda s: {int(k): float(v) for k, v in (kv.split(":") for kv in s.strip("{}").split(","))},
                            default={0: 0.1, 3: 0.8})
        elif f.name == "scale_range":
            ap.add_argument(flag, type=lambda s: tuple(float(x) for x in s.strip("()").split(",")), default=(1.0, 0.5))
        elif f.name == "output_path":
            ap.add_argument(flag, type=Path, default=Path("./outputs"))
        elif f.default is dataclasses.MISSING and f.default_factory is dataclasses.MISSING:
            ap.add_argument(flag, type=str, required=True)
        else:
            ap.add_argument(flag, type=type(f.default), default=f.default)
    return RunConfig(**vars(ap.parse_args(argv)))


def main(argv=None):
    config = _parse_cli(sys.argv[1:] if argv is None else argv)
    setup(config)
    register_builtin_losses()  # toLeftOf as the reference's main() does (run.py:240), and the other three directions
    if config.interactive:   # reference run.py:242-244
        from . import gui
        gui.run()
    else:
        execute(config)


if __name__ == "__main__":
    main()
