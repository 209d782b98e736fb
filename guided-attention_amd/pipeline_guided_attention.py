"""`GuidedAttention` — the per-step guided-attention sampling loop with the reference's interface
(pipeline_guided_attention.py:37-1123), host code in Python over the HIP kernels of libga_hip.so:

  per denoising step (reference :925-1053)
    A. guidance pass (autograd on):  UNet(latents, t, cond) with the capture processors  -> K1 x 32
       aggregate the 16x16 cross maps (K2) -> smoothed box loss (K3+K4) -> thresholds (host)
       iterative refinement / gradient step: autograd back to the latents (K1 bwd, K3+K4 bwd),
       latents <- latents - step * grad (K5)
    B. CFG pass (no grad):  UNet([latents]*2, t, [uncond, cond]) -> fused CFG combine + DDIM step
    C. recurse: re-noise back to level t (K6) and repeat while the step keeps updating

Kept from the reference: class name (`GuidedAttention`, alias `GuidedAttentionPipeline`), the
`__call__` keyword surface, the method names of the loss path and their return conventions, the use
of `utils.shared_state` globals, the control flow including its quirks (the second threshold test
reads the pre-refinement losses, :999).  Not reproduced (side effects off the path, declared in
DESIGN.md): per-token PNG dumps, predicted-x0 PNGs for steps 0-2, latent statistics logging,
deep-feature optimisation, the safety checker.
"""
import dataclasses
import json
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import ops
from ._lib import GaError
from .scheduler import DDIMScheduler
from .utils import helpers
from .utils import shared_state as state
from .utils import ptp_utils
from .utils.ptp_utils import AttentionStore, aggregate_attention, stored_maps

TERM = {"max_loss": 0, "col": 1, "row": 2, "inside_loss": 3, "outside_loss": 4, "token_loss": 5, "unscaled": 6}


class FusedRelation:
    """Stands where a plugin's loss tensor stands in the loss parts (`custom`) when the relation was evaluated inside the loss
    launch (GuidedAttention.fused_relation_loss): the differentiable loss of the parts already contains it; `value` is the
    relation part on the device ((1,), not differentiable)."""

    def __init__(self, value):
        self.value = value


class PipelineOutput(SimpleNamespace):
    """`.images`, `.nsfw_content_detected`, plus `.latents`, `.unet_calls` (run-time call counters) and `.variance_draws` (how
    many variance-noise tensors the call's CFG + DDIM steps consumed: 0 at eta = 0).  A call with num_images_per_prompt = S > 1
    or with guidance_states adds `.unet_calls_per_image` (S dicts), `.batched_passes` and `.logs` (S lists); its
    `.variance_draws` is a list of S counts."""


def draw_variance_noise(source, shape, dtype, device, where="the call"):
    """The variance noise of one CFG + DDIM step with eta > 0, (shape) on `device`: the next tensor of `source` when that is a
    list (host tensors handed to the call as `variance_noise`; an empty list is a ValueError naming `where`), else one
    torch.randn draw from the generator `source` on the generator's device (None: the global generator of `device`)."""
    if isinstance(source, list):
        if not source:
            raise ValueError(f"variance_noise ran out at {where}: one tensor per CFG step (recurse rounds add steps)")
        z = source.pop(0)
        if tuple(z.shape) != tuple(shape):
            raise ValueError(f"variance_noise at {where} is {tuple(z.shape)}, the latents are {tuple(shape)}")
        return z.to(device=device, dtype=dtype)
    gdev = source.device if source is not None else device
    return torch.randn(tuple(shape), generator=source, device=gdev, dtype=dtype).to(device)


@dataclass
class GuidanceState:
    """What one prompt of a call with `guidance_states` is guided by — what a solo call reads from the `utils.shared_state`
    globals.  `config`: what shared_state.config holds for that prompt after run.overrideConfig + run.parseMetaPrompt
    (prompt, token_dict, thresholds, only_update_on_threshold_steps, sub_prompt_avg_within, custom_loss, diagnostic_level,
    meta_prompt / meta_info); `hyper_params`: what shared_state.curHyperParams holds (strict, the loss scales, shrink_factor,
    bb_center_weight, recurse_steps, recurse_until, ...)."""
    config: Any
    hyper_params: Dict[str, Any]


def install_kernels(module, library_kernels=()):
    """The product's kernel choice on a module on the GPU — the UNet (GuidedAttention.to), or any block of it standing alone
    (the block-level tests), which then runs exactly what the pipeline installs.  `library_kernels`: see GuidedAttention.to."""
    from . import fused_linear
    from .unet import UNet2DConditionModel, set_fused_impl, set_norm_impl
    p = next(module.parameters())
    # MI355X layout: activations and conv weights channels-last end to end (MIOpen's NHWC kernels without
    # transposes) and the fused NHWC GroupNorm(+SiLU) HIP kernels in every norm layer
    module.to(memory_format=torch.channels_last)
    set_norm_impl(module, ops.group_norm_act)
    # `library_kernels` (A/B runs and the own-vs-library tests set it before .to()): the kinds named there — "conv",
    # "linear", "cat" — stay on MIOpen / hipBLASLt + the separate LayerNorm, GEGLU and add launches / torch.cat; default:
    # the package's own kernels for all three (16-bit dtypes; fp32 keeps the library)
    lib = set(library_kernels)
    conv = None if "conv" in lib else ops.conv3x3
    linear = None if "linear" in lib else fused_linear
    ops.prepare_device(p.device)   # split-K slabs / tickets exist before any hipGraph capture
    cat = None if "cat" in lib else ops.cat_channels
    set_fused_impl(module, ops.geglu, ops.bias_residual_add, (ops.layer_norm, ops.add_layer_norm), conv, linear, cat)
    # conv_in / conv_out and conv_in's backward to the latents: own kernels (csrc/thin_conv.hip) with the "conv" kind
    for m in module.modules():
        if isinstance(m, UNet2DConditionModel):
            m.edge_conv_impl = (ops.conv3x3_thin_apply if conv is not None and
                                m.dtype in (torch.float16, torch.bfloat16) else None)
    # MIOpen's exhaustive search (cudnn.benchmark) stays OFF.  It executes every candidate solver once per shape, and a
    # candidate of the backward-data search for conv_in (4 <- 64 channels, 32 x 32, fp16) reads past its operands: a GPU
    # memory access fault that killed the process whenever the tensors happened to sit at the end of a mapped segment
    # (round 4, deterministic in `pytest tests/test_pipeline_gpu.py`, the worker thread in a native autograd node:
    # profiles/r4_fault_half_precision_graphs_wide.log; round 3 had seen "the fp32 96x96 backward-data search abort
    # the process once").  Only the three stride-2 backward convolutions (and the edge convolutions of shapes the own
    # kernels do not serve) are still on the library.
    torch.backends.cudnn.benchmark = False


class GuidedAttention:
    vae_scale_factor = 8

    def __init__(self, unet, scheduler=None, vae=None, text_encoder=None, tokenizer=None):
        self.unet = unet
        self.scheduler = scheduler or DDIMScheduler()
        self.vae = vae
        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        self.prompt = None
        self.inside_iterative_refinement = False
        # "full": run the whole UNet in the guidance pass, as the reference does.  "truncated": stop after the
        # last attention map the loss reads (up_blocks.1): identical latents, fewer FLOPs (declared when used).
        self.guidance_forward = "full"
        # False keeps the reference's behaviour of evaluating the guidance pass + loss on every step even when
        # no update can follow (steps outside `thresholds` with only_update_on_threshold_steps): log-only work.
        self.skip_unused_guidance = False
        # True: the two UNet passes are captured once into hipGraphs (guidance forward + loss, its backward, the CFG
        # forward) and replayed — same kernels, no per-launch host work.  False: eager launches.
        self.use_graphs = False
        # With hipGraphs: on steps where no latent update can follow the guidance evaluation (its loss is only
        # logged), run the guidance forward (cond) and the CFG pair (uncond, cond) — three independent evaluations of
        # the same latents — as ONE batch-3 pass.  Nothing is skipped; False runs them as two passes (B=1, B=2).
        self.batch_loss_only_guidance = True
        # The reference writes per-token attention-map PNGs at EVERY loss evaluation (:243-246), predicted-x0 PNGs for the
        # steps in shared_state.always_save_iter (:1036-1037) and latent statistics at every step (:1031), whatever
        # config.diagnostic_level says.  Here those side effects are opt-in: True reproduces them (each costs device
        # syncs and host I/O; hipGraph replay is bypassed for such a run).  config.diagnostic_level > 0 switches them on
        # as well.  Off by default, never inside a timed benchmark region.
        self.reference_side_effects = False
        self.library_kernels = frozenset()   # see .to()
        # With hipGraphs, inside the iterative refinement: enqueue an iteration's backward, latent update and the NEXT guidance
        # evaluation before reading the iteration's loss table back.  Nothing is speculative about WHAT runs — the update is
        # unconditional whenever the loss is not exactly 0 (reference :551), and whatever the threshold test says afterwards the
        # next launch is an evaluation of the updated latents (the next iteration's, or the final one, :566) — only about the
        # `loss != 0` test, whose other outcome discards and repeats (never counted).  False: enqueue, read, decide, enqueue.
        self.speculative_refinement = True
        # True: a call with num_images_per_prompt > 1 or guidance_states serves paint-with-words (paint_with_words_stop > 0) per
        # image — each image's own score maximum, mask and multiplier (ga_attn_*_grouped).  Such a call runs eager, without
        # hipGraphs and joint passes, as a solo paint-with-words call does.  A declared variant, off until it runs under graphs:
        # False refuses such a call.
        self.batched_paint_with_words = False
        # True: `[CustomLoss:toLeftOf (a, b)]`, toRightOf, above, below — a custom-loss set whose plugins are all run.ToLeftOf,
        # ToRightOf, Above or Below themselves — is evaluated inside
        # the loss launches (ga_aggregate_loss_rel_fwd_images / ga_smooth_loss_rel_bwd_images: one launch each way instead of the
        # two-launch loss plus the plugin's torch graph), and batched calls serve it per image.  Any other plugin keeps the
        # plugin path in a solo call and the refusal in a batched one.  A declared variant, off by default.
        self.fused_relation_loss = False
        # True: a call with num_images_per_prompt > 1 or guidance_states serves `use_optimizer` (the refinement loop's SGD with
        # momentum) per image: the images that step share one backward pass with the images that take a plain update, then
        # ga_latent_sgd_momentum_batched steps them (per-image lr, first-step flag and velocity slice).  A declared variant, off
        # by default: False refuses such a call.
        self.batched_momentum_refinement = False
        # True: decode_latents (output_type="pil", save_image) runs the VAE decoder on the package's own kernels
        # (vae.AutoencoderKLDecoder.decode_own: ga_latent_affine4, the UNet's convolution / GroupNorm / Linear kernels,
        # ga_attn_wide_fwd for the 512-wide mid-block attention), channels-last, in chunks of at most vae.decode_chunks images.
        # 16-bit pipelines on the GPU only: fp32 and CPU pipelines keep the framework path whatever the switch says.  A
        # declared variant, off by default: False is vae.decode as one framework launch sequence.
        self.own_vae_decode = False
        self.vae_decode_budget = None   # elements of the largest activation of one decode chunk; None: vae.MAX_CHUNK_ELEMS
        self._runner = None
        self._graph_cache = {}
        self.unet_calls = {"fwd_b1_grad": 0, "bwd": 0, "fwd_b2": 0, "loss_evals": 0, "joint_b3": 0}
        self._plan_key = None
        self._plan = None
        self._deferred_log, self._deferred_losses = [], []   # a batched call may come first: _resume swaps these

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(cls, name_or_path, revision=None, torch_dtype=None, random_init=False, unet_config=None,
                        seed=0, weights=True, **kwargs):
        """Local diffusers-layout folder -> weights loaded by name.  There is no network here: an id that is
        not a local folder raises unless random_init=True, which builds seeded random weights of the named
        architecture (SD-1.x for anything but '*2-1*').  weights=False builds the architecture only (no file read,
        no random draw): what the ranks other than 0 do before the weight broadcast (run.load_model).  A local folder's
        scheduler/scheduler_config.json (prediction_type, num_train_timesteps, beta_start, beta_end, steps_offset,
        set_alpha_to_one; beta_schedule must be scaled_linear) and the sample_size of its unet/config.json (when no unet_config
        is passed) are read where they exist."""
        from pathlib import Path
        from .text import SyntheticTextEncoder, WordTokenizer, load_clip
        from .unet import UNet2DConditionModel, UNetConfig
        from .vae import AutoencoderKLDecoder
        sd21 = "2-1" in str(name_or_path)
        folder = Path(str(name_or_path))
        cfg = unet_config or (UNetConfig.sd21(sample_size=64) if sd21 else UNetConfig.sd15())
        scheduler = DDIMScheduler()
        if folder.is_dir() and (folder / "unet").is_dir():
            from safetensors.torch import load_file
            # the checkpoint's own settings, where its folder states them: the latent side (the 768 checkpoints say 96) and the
            # DDIM schedule with its prediction type (SD-2.1 768-v: v_prediction); no file, today's defaults
            unet_json = folder / "unet" / "config.json"
            if unet_config is None and unet_json.is_file():
                side = json.loads(unet_json.read_text()).get("sample_size")
                if side is not None:
                    cfg = dataclasses.replace(cfg, sample_size=int(side))
            scheduler = cls._scheduler_from_folder(folder)
            unet = UNet2DConditionModel(cfg)
            if weights:
                unet.load_diffusers_state(load_file(str(folder / "unet" / "diffusion_pytorch_model.safetensors")))
            vae = AutoencoderKLDecoder()
            vae_file = folder / "vae" / "diffusion_pytorch_model.safetensors"
            if vae_file.exists() and weights:
                sd = {k: v for k, v in load_file(str(vae_file)).items()
                      if k.startswith(("decoder.", "post_quant_conv."))}
                vae.load_state_dict(sd, strict=False)
            clip = load_clip(folder)
            tok, enc = clip if clip else (WordTokenizer(), SyntheticTextEncoder(cfg.cross_attention_dim))
        elif random_init:
            unet = UNet2DConditionModel(cfg)
            small = cfg.block_out_channels[0] < 128
            vae = AutoencoderKLDecoder.tiny() if small else AutoencoderKLDecoder()
            if weights:
                unet.init_weights_(seed)
                vae.init_weights_(seed + 1)
            tok, enc = WordTokenizer(pad_token_id=0 if sd21 else 49407), SyntheticTextEncoder(cfg.cross_attention_dim)
        else:
            raise FileNotFoundError(f"{name_or_path!r} is not a local checkpoint folder and there is no network; "
                                    "pass random_init=True for seeded random weights of that architecture")
        pipe = cls(unet, scheduler, vae, enc, tok)
        dtype = torch_dtype or (torch.float16 if revision == "fp16" else None)
        if dtype is not None:
            pipe.to(dtype=dtype)
        return pipe

    @staticmethod
    def _scheduler_from_folder(folder):
        """The DDIMScheduler a checkpoint folder's scheduler/scheduler_config.json describes (diffusers layout); the defaults
        where there is no file.  Only the scaled-linear beta schedule is built here: another one is refused, not approximated."""
        path = folder / "scheduler" / "scheduler_config.json"
        if not path.is_file():
            return DDIMScheduler()
        conf = json.loads(path.read_text())
        schedule = conf.get("beta_schedule", "scaled_linear")
        if schedule != "scaled_linear":
            raise ValueError(f"{path}: beta_schedule {schedule!r}; the DDIM scheduler here builds 'scaled_linear' only")
        return DDIMScheduler.from_config(conf)

    def to(self, device=None, dtype=None):
        for m in (self.unet, self.vae, self.text_encoder):
            if m is not None:
                m.to(device=device, dtype=dtype)
        for p in self.unet.parameters():
            p.requires_grad_(False)  # only the latents are differentiated (reference :466)
        if self.unet.device.type == "cuda":
            install_kernels(self.unet, self.library_kernels)
            from . import fused_linear
            from .vae import AutoencoderKLDecoder, set_own_kernels
            if isinstance(self.vae, AutoencoderKLDecoder):
                set_own_kernels(self.vae, ops, fused_linear)   # handles only: vae.decode stays the framework path
        return self

    @property
    def device(self):
        return self.unet.device

    _execution_device = device

    # ------------------------------------------------------------------ prompt side
    def _encode_prompt(self, prompt, device, num_images_per_prompt, do_classifier_free_guidance,
                       negative_prompt=None, prompt_embeds=None, negative_prompt_embeds=None):
        """-> (text_inputs, cat[negative, positive] embeddings)  (reference :64-199)."""
        text_inputs = None
        batch_size = 1 if isinstance(prompt, str) else (len(prompt) if prompt is not None else prompt_embeds.shape[0])
        if prompt_embeds is None:
            text_inputs = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length,
                                         truncation=True, return_tensors="pt")
            prompt_embeds = self.text_encoder(text_inputs.input_ids.to(device))[0]
        prompt_embeds = prompt_embeds.to(dtype=self.unet.dtype, device=device)
        b, n, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(b * num_images_per_prompt, n, -1)
        if do_classifier_free_guidance:
            if negative_prompt_embeds is None:
                if negative_prompt is None:
                    uncond = [""] * batch_size
                elif isinstance(negative_prompt, str):
                    uncond = [negative_prompt]
                else:
                    if batch_size != len(negative_prompt):
                        raise ValueError("`negative_prompt` batch size does not match `prompt`")
                    uncond = negative_prompt
                ids = self.tokenizer(uncond, padding="max_length", max_length=prompt_embeds.shape[1], truncation=True,
                                     return_tensors="pt").input_ids
                negative_prompt_embeds = self.text_encoder(ids.to(device))[0]
            negative_prompt_embeds = negative_prompt_embeds.to(dtype=self.unet.dtype, device=device)
            n = negative_prompt_embeds.shape[1]
            negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1).view(
                batch_size * num_images_per_prompt, n, -1)
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds])
        return text_inputs, prompt_embeds

    def check_inputs(self, prompt, height, width, callback_steps, negative_prompt=None, prompt_embeds=None,
                     negative_prompt_embeds=None):
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_steps is None or not isinstance(callback_steps, int) or callback_steps <= 0:
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps}.")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError("Cannot forward both `prompt` and `prompt_embeds`.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        if prompt is not None and not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        shape = (batch_size, num_channels_latents, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if latents is None:
            gdev = generator.device if generator is not None else device
            latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
        else:
            if tuple(latents.shape) != shape:
                raise ValueError(f"Unexpected latents shape, got {tuple(latents.shape)}, expected {shape}")
            latents = latents.to(device=device, dtype=dtype)
        return latents * self.scheduler.init_noise_sigma

    def _decode_own(self, latents):
        """The decoder on own kernels (own_vae_decode): scale + post_quant_conv in ga_latent_affine4, then vae.decode_own, in
        chunks whose largest activation the kernels' 32-bit offsets hold (vae.decode_chunks)."""
        from .vae import MAX_CHUNK_ELEMS, decode_chunks
        if not hasattr(self.vae, "decode_own"):
            raise ops.GaError("own_vae_decode needs vae.AutoencoderKLDecoder (decode_own); this VAE has no own-kernel forward")
        S, _, h, w = latents.shape
        chunks = decode_chunks(S, h, w, self.vae.ch, self.vae_decode_budget or MAX_CHUNK_ELEMS)
        parts = [self.vae.decode_own(latents[a:b], 1.0 / self.vae.scaling_factor) for a, b in chunks]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def decode_latents(self, latents):
        dtype = self.unet.dtype
        if self.own_vae_decode and latents.is_cuda and dtype in (torch.float16, torch.bfloat16):
            image = self._decode_own(latents.to(dtype))
        else:
            image = self.vae.decode(latents.to(dtype) / self.vae.scaling_factor)
        image = (image / 2 + 0.5).clamp(0, 1)
        return image.detach().cpu().permute(0, 2, 3, 1).float().numpy()

    @staticmethod
    def numpy_to_pil(images):
        from PIL import Image
        if images.ndim == 3:
            images = images[None]
        return [Image.fromarray(im) for im in (images * 255).round().astype("uint8")]

    def get_token(self, index):
        return self.tokenizer.decode(self.tokenizer(state.config.prompt)["input_ids"][index])

    # ------------------------------------------------------------------ the loss path (HIP)
    def _loss_plan(self, smooth, sigma, kernel_size):
        td = state.config.token_dict
        hp = state.curHyperParams
        entries = []
        for idx, info in td.items():
            if info["loss_type"] == helpers.AnnotationType.BOX:
                entries.append({"index": idx, "kind": "BOX", "geom": tuple(float(v) for v in info["loss"].as_tuple()),
                                "subprompt": info["subprompt"]})
            elif info["loss_type"] == helpers.AnnotationType.COOR:
                entries.append({"index": idx, "kind": "COOR", "geom": tuple(float(v) for v in info["loss"]),
                                "subprompt": info["subprompt"]})
            else:  # KEYWORD tokens only mark sub-prompts for custom losses: no built-in term
                continue
        # keyed on CONTENT (token positions, kinds, geometry, sub-prompts, the hyper-parameters the plan reads): an
        # in-place edit of a Rect invalidates the plan (the captured hipGraphs bake the geometry in by value), and a
        # fresh but equal token_dict — run.execute builds one per (seed, hyper-parameter state) — reuses plan and graphs
        key = (tuple((e["index"], e["kind"], e["geom"], e["subprompt"]) for e in entries),
               tuple((idx, info["loss_type"].name) for idx, info in td.items()),
               smooth, sigma, kernel_size, state.config.sub_prompt_avg_within,
               tuple(sorted((k, str(v)) for k, v in hp.items() if k in ops.LossPlan.HYPER_KEYS)))
        if key != self._plan_key:
            self._plan = ops.LossPlan(entries, hp, smooth, sigma, kernel_size, state.config.sub_prompt_avg_within)
            self._plan_key = key
        return self._plan

    # ------------------------------------------------------------------ the directional relations in the loss launches
    @staticmethod
    def _relation_kinds():
        """plugin class -> (ga_relation_t.kind, the relation's prompt name) of the four relations the loss launches serve"""
        from . import _lib, run
        return {run.ToLeftOf: (_lib.GA_REL_LEFT_OF, "toLeftOf"), run.ToRightOf: (_lib.GA_REL_RIGHT_OF, "toRightOf"),
                run.Above: (_lib.GA_REL_ABOVE, "above"), run.Below: (_lib.GA_REL_BELOW, "below")}

    def _relations_eligible(self, custom):
        """A custom-loss set the loss launches serve: the switch is on and every plugin is run.ToLeftOf, ToRightOf, Above or
        Below itself (a subclass may override calc_loss)."""
        if not (self.fused_relation_loss and custom):
            return False
        kinds = self._relation_kinds()
        return all(type(fn) in kinds for fn, _args in custom.values())

    def _relation_plan(self):
        """shared_state.config.custom_loss as an ops.RelationPlan (None: no custom loss, or not eligible).  The slice indices are
        what the plugin itself would read: find_indices_for_sub_prompt of both sub-prompts; one that does not resolve raises
        ValueError here, on the host, where the plugin would fail inside calc_loss."""
        custom = getattr(state.config, "custom_loss", None)
        if not self._relations_eligible(custom):
            return None
        kinds = self._relation_kinds()
        relations = []
        for _name, (fn, args) in custom.items():
            kind, name = kinds[type(fn)]
            subs = fn.parse_text_args(fn.quote_items_in_tuple(args))
            if len(subs) != 2:
                raise ValueError(f"{name} takes two sub-prompts, got {args!r}")
            sides = []
            for sub in subs:
                idx = fn.find_indices_for_sub_prompt(sub)
                if not idx:
                    raise ValueError(f"{name} {args}: sub-prompt {sub!r} is not part of the prompt {state.config.prompt!r}")
                sides.append(idx)
            relations.append((sides[0], sides[1], kind))   # a's indices, b's indices: the kernels apply the role from the kind
        return ops.RelationPlan(relations)

    def _check_relations(self, cfg):
        """Before any launch: cfg's eligible custom losses must resolve (ValueError naming the sub-prompt otherwise)."""
        saved = state.config
        state.config = cfg
        try:
            self._relation_plan()
        finally:
            state.config = saved

    def _solo_relation_table(self, attention_res, smooth, sigma, kernel_size, last_idx):
        """The one-row table (loss row + relation row) of a solo call whose custom losses the loss launches serve, or None.
        The pipeline owns one table per (capacities, call-level loss settings): captured graphs read its buffers, `set` refills
        them only when the rows change — so __call__ fills it before the first launch (and before any capture)."""
        if self._dump or not self.fused_aggregate_loss or self._images > 1 or self._table is not None:
            return None
        custom = getattr(state.config, "custom_loss", None)
        if not self._relations_eligible(custom):
            return None
        plan = self._loss_plan(smooth, sigma, kernel_size)
        key = (self._plan_key, tuple((n, id(fn), str(a)) for n, (fn, a) in sorted(custom.items())), str(state.config.prompt),
               attention_res, last_idx, str(self.device))
        if key == self._rel_key:
            return self._rel_table
        rel = self._relation_plan()
        T_max, Q_max = ops.image_table_capacity(plan.T), ops.relation_capacity(len(rel.columns))
        tkey = ("solo relation", T_max, Q_max, attention_res, bool(smooth), float(sigma), int(kernel_size), str(self.device))
        tables = self.__dict__.setdefault("_image_tables", {})
        if tkey not in tables:
            tables[tkey] = ops.ImageTable(1, T_max, attention_res, smooth, sigma, kernel_size, self.device, Q_max=Q_max)
        self._rel_table = tables[tkey].set([plan], [(1, last_idx)], [rel])
        self._rel_key = key
        return self._rel_table

    _rel_key = _rel_table = None

    def _last_text_index(self, n_tok, normalize_eot):
        if normalize_eot:
            prompt = self.prompt[0] if isinstance(self.prompt, list) else self.prompt
            return len(self.tokenizer(prompt)["input_ids"]) - 1
        return n_tok - 1

    def _aggregate_loss_device(self, attention_store, attention_res, smooth_attentions, sigma, kernel_size, normalize_eot):
        """aggregate_attention + the loss evaluation, device half.  The common case — built-in box / coordinate terms
        only, no diagnostics — is ONE launch (ga_aggregate_loss_fwd: the head-map mean never makes its own pass and its
        backward is one launch as well); custom Python losses and the PNG dumps need the aggregate as a differentiable
        tensor of its own and take the two-step form.  Results are identical (GPU test).  With fused_relation_loss, a prompt
        whose custom losses are all directional relations (_relations_eligible) is ONE launch as well (the table form with a relation row)."""
        if self._table is not None:   # images of different prompts / layouts: one descriptor row per image
            S = self._images
            maps = stored_maps(attention_store, attention_res, ("up", "down", "mid"), True, 0)
            if self._table.Q_max:   # some image has a relation: box + relation in the same launch, one (box, relation) pair per row
                _, terms, box, _, rel, total = ops.AggregateSmoothLossRelImages.apply(self._table, *maps)
                packed = torch.cat([terms.reshape(S, -1), box.reshape(S, 1), rel.reshape(S, 1)], dim=1)
                return terms, total, FusedRelation(rel), self._table, packed
            _, terms, loss = ops.AggregateSmoothLossImages.apply(self._table, *maps)
            packed = torch.cat([terms.detach().reshape(S, -1), loss.detach().reshape(S, 1), loss.new_zeros(S, 1)], dim=1)
            return terms, loss, None, self._table, packed
        plan = self._loss_plan(smooth_attentions, sigma, kernel_size)
        custom = getattr(state.config, "custom_loss", None)
        if self._images == 1 and self._relations_eligible(custom):
            maps = stored_maps(attention_store, attention_res, ("up", "down", "mid"), True, 0)
            last_idx = self._last_text_index(maps[0].shape[-1], normalize_eot)
            table = self._solo_relation_table(attention_res, smooth_attentions, sigma, kernel_size, last_idx)
            if table is not None:   # the relation inside the one loss launch (also with T = 0: every token a KEYWORD)
                _, terms, box, _, rel, total = ops.AggregateSmoothLossRelImages.apply(table, *maps)
                packed = torch.cat([terms[0, :plan.T].reshape(-1), box, rel])
                return terms[0, :plan.T], total, FusedRelation(rel), plan, packed
        if self._images > 1:   # S images: one batched launch each way; packed = one row per image
            S = self._images
            maps = stored_maps(attention_store, attention_res, ("up", "down", "mid"), True, 0)
            last_idx = self._last_text_index(maps[0].shape[-1], normalize_eot)
            _, terms, loss = ops.AggregateSmoothLossBatched.apply(S, attention_res, 1, last_idx, plan, *maps)
            packed = torch.cat([terms.detach().reshape(S, -1), loss.detach().reshape(S, 1), loss.new_zeros(S, 1)], dim=1)
            return terms, loss, None, plan, packed
        if plan.T > 0 and not custom and not self._dump and self.fused_aggregate_loss:
            maps = stored_maps(attention_store, attention_res, ("up", "down", "mid"), True, 0)
            last_idx = self._last_text_index(maps[0].shape[-1], normalize_eot)
            _, terms, loss = ops.AggregateSmoothLoss.apply(attention_res, 1, last_idx, plan, *maps)
            packed = torch.cat([terms.detach().reshape(-1), loss.detach(), loss.new_zeros(1)])
            return terms, loss, None, plan, packed
        attention_maps = aggregate_attention(attention_store=attention_store, res=attention_res,
                                             from_where=("up", "down", "mid"), is_cross=True, select=0)
        if self._dump and getattr(state.config, "save_individual_CA_maps", False) and state.cur_time_step_iter == 12:
            self._dump_individual_ca_maps(attention_store, attention_maps, ("up", "down", "mid"))
        return self._loss_device(attention_maps, smooth_attentions, sigma, kernel_size, normalize_eot)

    fused_aggregate_loss = True   # False: always aggregate_attention + loss as two launches (A/B and parity tests)
    _images = 1                   # S while a batched call (num_images_per_prompt = S > 1) runs
    _table = None                 # the ops.ImageTable while a call with guidance_states runs

    def _loss_device(self, attention_maps, smooth_attentions, sigma, kernel_size, normalize_eot):
        """Device half of the loss evaluation (graph-capturable: no host sync): -> (terms, loss, custom, plan)."""
        res, n_tok = attention_maps.shape[0], attention_maps.shape[-1]
        last_idx = self._last_text_index(n_tok, normalize_eot)
        plan = self._loss_plan(smooth_attentions, sigma, kernel_size)
        if plan.T > 0:
            terms, loss = ops.SmoothLoss.apply(attention_maps.reshape(res * res, n_tok), res, 1, last_idx, plan)
        else:  # every annotated token is a KEYWORD of a custom loss (reference: no built-in term, :409-438)
            terms = attention_maps.new_zeros((0, 8))
            loss = attention_maps.new_zeros(1)
        custom = None
        if self._dump:
            self._dump_token_maps(attention_maps, last_idx)
        if hasattr(state.config, "custom_loss") and state.config.custom_loss:
            text_maps = torch.softmax(attention_maps[:, :, 1:last_idx] * 100, dim=-1)
            for _name, (fn, args) in state.config.custom_loss.items():
                v = fn.calc_loss(text_maps, args)
                custom = v if custom is None else custom + v
        # everything the host tests in ONE device->host copy: the term table, the fused loss and the custom-loss value
        cval = custom.detach().float().reshape(-1)[:1] if custom is not None else loss.new_zeros(1)
        packed = torch.cat([terms.detach().reshape(-1), loss.detach(), cval])
        return terms, loss, custom, plan, packed

    def _loss_host(self, terms, loss, custom, plan, packed):
        """Host half: the one device sync per evaluation (the thresholds need the values), then the reference's
        `losses_dict` keys (one entry per guided token) plus the fused results."""
        self.unet_calls["loss_evals"] += 1
        host = packed.cpu()
        host_terms = host[:-2].view(plan.T, 8)
        losses_dict = {k: [terms[t, c] for t in range(plan.T)] for k, c in TERM.items() if c < 5}
        # host_total = the value the reference tests with `loss != 0` (:551, :1002): box terms plus custom loss
        losses_dict["_fused"] = {"loss": loss, "host_terms": host_terms, "host_loss": host[-2:-1], "plan": plan,
                                 "host_custom": host[-1:], "host_total": host[-2:-1] + host[-1:],
                                 "relation_fused": isinstance(custom, FusedRelation)}
        if custom is not None:
            losses_dict["custom_loss"] = custom
        for t, e in enumerate(plan.entries):
            word = state.config.token_dict[e["index"]]["word"]
            helpers.log(f"{word}: weighted center col {host_terms[t, 1].item()} row {host_terms[t, 2].item()}")
        return losses_dict

    def _compute_max_attention_per_index(self, attention_maps, smooth_attentions=False, sigma=0.5, kernel_size=3,
                                         normalize_eot=False):
        """attention_maps (res, res, n_tokens) f32 -> losses_dict with the reference's keys plus the fused
        results of ga_smooth_loss_fwd (reference :201-296)."""
        return self._loss_host(*self._loss_device(attention_maps, smooth_attentions, sigma, kernel_size, normalize_eot))

    _dump = False  # True while a run reproduces the reference's PNG / log side effects (set per __call__)

    # ------------------------------------------------------------------ diagnostics (reference :243-246, 316-346, 1090-1123)
    def get_innermost_folder(self):
        return str(state.cur_seed)

    def _dump_dir(self):
        d = state.config.output_path / helpers.get_inner_folder_name() / self.get_innermost_folder()
        d.mkdir(exist_ok=True, parents=True)
        return d

    def save_viridis(self, tensor1, tag):
        """Min-max normalised map as a viridis PNG (reference :1096-1103)."""
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        with torch.no_grad():
            x = tensor1.float() - tensor1.float().min()
            x = x / x.max()
            fname = (tag + "_" + helpers.get_meta_prompt_clean() + state.get_name() + "_subiter_" +
                     "{:02d}".format(state.sub_iteration) + ".png")
            plt.imsave(self._dump_dir() / fname, x.detach().cpu().numpy())

    def save_numpy(self, tensor1, tag):
        fname = tag + "_" + helpers.get_meta_prompt_clean() + "_" + str(state.cur_time_step_iter)
        np.save(self._dump_dir() / fname, tensor1.detach().float().cpu().numpy())

    def save_image(self, latent, tag):
        """Decode latents and save the (annotated) image (reference :1114-1123)."""
        image = self.numpy_to_pil(self.decode_latents(latent.detach()))
        fname = helpers.get_meta_prompt_clean() + state.get_name() + "_" + tag
        for ch in "[]:.":
            fname = fname.replace(ch, "_")
        helpers.annotate_image(image[0])
        image[0].save(self._dump_dir() / (fname + ".png"))

    def _dump_token_maps(self, attention_maps, last_idx):
        """Per-token maps of softmax(100 * A[:, :, 1:last]) as PNGs + their sums in the log (reference :238-246)."""
        with torch.no_grad():
            text = torch.softmax(attention_maps.detach()[:, :, 1:last_idx] * 100, dim=-1)
            if getattr(state.config, "save_all_maps", False):
                indices = range(0, len(self.tokenizer(state.config.prompt)["input_ids"][1:-1]))
            else:
                indices = [index - 1 for index in state.config.token_dict.keys()]
            for index_i in indices:
                image = text[:, :, index_i]
                self.save_viridis(image, "_attnmap_" + self.get_token(index_i + 1))
                helpers.log(self.get_token(index_i + 1) + ": " + str(image.sum().item()))

    def _dump_individual_ca_maps(self, attention_store, attention_maps, from_where):
        """config.save_individual_CA_maps at step 12: every head of every stored cross map (token 1), the head mean
        and the aggregate (reference :316-346)."""
        for location in from_where:
            for map_iter, item in enumerate(attention_store.get_average_attention()[f"{location}_cross"], start=1):
                if not torch.is_tensor(item):
                    continue
                res = int(item.shape[1] ** .5)
                cross_maps = item.reshape(-1, res, res, item.shape[-1])
                for head in range(0, min(8, cross_maps.shape[0])):
                    map1 = cross_maps[head, :, :, 1]
                    tag = (f"{location}_res_{res}_head_{head}_mapiter_{map_iter}_avg_{map1.mean().item():.3}"
                           f"_max_{map1.max().item():.3}")
                    self.save_viridis(map1, tag)
                self.save_viridis((cross_maps.sum(0) / 8)[:, :, 1], f"{location}_res_{res}_avgheads_mapiter_{map_iter}")
        self.save_viridis(attention_maps[:, :, 1], "final")

    def _aggregate_and_get_max_attention_per_token(self, attention_store, attention_res=16, smooth_attentions=False,
                                                   sigma=0.5, kernel_size=3, normalize_eot=False):
        return self._loss_host(*self._aggregate_loss_device(attention_store, attention_res, smooth_attentions, sigma,
                                                            kernel_size, normalize_eot))

    @staticmethod
    def group_losses_by_sumprompt(losses):
        """[(token index | None, value)] -> (total, {sub-prompt: value}); sum within a sub-prompt, or the mean
        when config.sub_prompt_avg_within (reference :359-387).  fp32 accumulation like the reference's tensors."""
        groups = {}
        for tok, val in losses:
            sub = None if tok is None else state.config.token_dict[tok]["subprompt"]
            groups.setdefault(sub, []).append(val)
        total = None
        finals = {}
        for sub, vals in groups.items():
            acc = None
            for v in vals:
                v = v.float() if torch.is_tensor(v) else torch.tensor([float(v)])
                if state.config.sub_prompt_avg_within:
                    v = v / len(vals)
                acc = v if acc is None else acc + v
            finals[sub] = acc
            total = acc if total is None else total + acc
        if total is None:
            total = torch.zeros(1)
        return total, finals

    @staticmethod
    def get_centering_loss(center, losses_dict, i):
        res = 16
        part1 = (losses_dict["col"][i] - center[0] * res).abs() / (res - 1.)
        part2 = 4. * (losses_dict["row"][i] - center[1] * res).abs() / (res - 1.)
        return part1 + part2

    @staticmethod
    def _compute_loss(losses_dict, return_losses=False):
        """-> (loss (1,) on the device with grad, losses [(token, value)], unscaled_losses [(token, value)]).
        The per-token values are host-side fp32 scalars (already synchronised by the loss evaluation)."""
        fused = losses_dict["_fused"]
        host, plan = fused["host_terms"], fused["plan"]
        losses, unscaled = [], []
        for t, e in enumerate(plan.entries):
            info = state.config.token_dict[e["index"]]
            losses.append((e["index"], host[t, TERM["token_loss"]:TERM["token_loss"] + 1]))
            unscaled.append((e["index"], host[t, TERM["unscaled"]:TERM["unscaled"] + 1]))
            if info["loss_type"] == helpers.AnnotationType.BOX:
                helpers.log(f"{state.cur_time_step_iter:02d}.{state.sub_iteration:02d} loss for {info['word']}: "
                            f"{host[t, TERM['unscaled']].item()}")
        loss = fused["loss"]
        if "custom_loss" in losses_dict:
            custom = losses_dict["custom_loss"]
            losses.append((None, fused["host_custom"]))
            unscaled.append((None, fused["host_custom"]))
            if not fused.get("relation_fused"):   # evaluated inside the loss launch: `loss` is box + relation already
                loss = loss + custom.to(loss.dtype).reshape(1)
        return loss, losses, unscaled

    def meets_threshold(self, i, thresholds, losses):
        """reference :1074-1088 — every sub-prompt's (unscaled) loss must be <= the step's threshold."""
        _, per_sub = GuidedAttention.group_losses_by_sumprompt(losses)
        if (i not in thresholds and i != -1) or len(thresholds) == 0:
            return True
        thresh = list(thresholds.values())[-1] if i == -1 else thresholds[i]
        for val in per_sub.values():
            if bool(val > thresh):  # fp32 tensor vs Python float: compared in fp32, as in the reference
                return False
        return True

    # ------------------------------------------------------------------ the launches a driver answers requests with
    def _latent_gradient(self, latents, loss):
        """dLoss/dlatents: autograd back through the UNet (K1 / K3+K4 backward kernels inside), or one hipGraph replay of the
        captured backward pass when `loss` is the runner's."""
        runner = self._runner
        if runner is not None and loss is runner.loss:
            return runner.backward()
        grad = torch.autograd.grad(loss.requires_grad_(True), [latents], retain_graph=True)[0]
        ops.end_image_broadcasts()   # the relation launch's backward hands its map over through the image-broadcast table
        return grad

    def _update_latent(self, latents, loss, step_size):
        """latents - step_size * dLoss/dlatents (reference :456-470): the gradient, then the fused axpy + mean|grad| kernel.
        The counted single-call form; a driver applies the same two launches and leaves the counting to the program."""
        self.unet_calls["bwd"] += 1
        new_latents, absmean = ops.latent_axpy(latents.detach(), self._latent_gradient(latents, loss), float(step_size), True)
        self._deferred_log.append(("gradient size average: ", absmean))
        return new_latents

    def _momentum_step(self, latents, loss, momentum):
        """One optimizer step of the `use_optimizer` refinement (reference :549-551): the gradient as in _update_latent, then
        the fused velocity + latent update.  No `gradient size average` line: that one lives in _update_latent."""
        self.unet_calls["bwd"] += 1
        new_latents = ops.latent_sgd_momentum(latents.detach(), self._latent_gradient(latents, loss), momentum["velocity"],
                                              momentum["lr"], momentum["mu"], momentum["first"])
        momentum["first"] = False
        return new_latents

    def _guidance_forward(self, latents, t, cond, time_projection=None):
        if self.guidance_forward == "truncated" and self._truncate_at is not None:
            out = self.unet(latents, t, encoder_hidden_states=cond, stop_after_up_block=self._truncate_at,
                            time_projection=time_projection).sample
            if hasattr(self._attention_store, "flush"):
                self._attention_store.flush()
            return out
        return self.unet(latents, t, encoder_hidden_states=cond, time_projection=time_projection).sample

    def _guidance_parts(self, latents, t, cond, attention_store, attention_res, smooth_attentions, sigma, kernel_size,
                        normalize_eot):
        """Enqueue one guidance evaluation = restart the autograd graph at the latents, UNet forward with capture, aggregate,
        loss: eager, or one hipGraph replay.  -> (latents leaf the loss depends on, loss parts with the table still on the
        device).  With the runner the leaf is its ONE static buffer, which the next evaluation overwrites."""
        if self._runner is not None:
            return self._runner.evaluate(latents, t, attention_store)
        with torch.enable_grad():
            leaf = latents.detach().clone().requires_grad_(True)
            self._guidance_forward(leaf, t, cond)
            return leaf, self._aggregate_loss_device(attention_store, attention_res, smooth_attentions, sigma, kernel_size,
                                                     normalize_eot)

    def _guidance_eval(self, latents, t, cond, attention_store, attention_res, smooth_attentions, sigma, kernel_size,
                       normalize_eot):
        """One guidance evaluation, enqueued and read: -> (latents leaf the loss depends on, losses_dict)."""
        self.unet_calls["fwd_b1_grad"] += 1
        leaf, parts = self._guidance_parts(latents, t, cond, attention_store, attention_res, smooth_attentions, sigma,
                                           kernel_size, normalize_eot)
        return leaf, self._loss_host(*parts)

    @staticmethod
    def _loss_is_zero(losses_dict):
        return losses_dict["_fused"]["host_total"].item() == 0

    # ------------------------------------------------------------------ the guidance step: one program, two drivers
    def _guidance_step(self, i, t_int, thresholds, step_size, max_iter_to_alter, run_standard_sd, joint):
        """Denoising step i of one image (reference :925-1053) as a program: everything the reference decides on the host, its
        log lines and the call counters, and no device work.  It yields requests and is resumed (_resume) with the reply of
        whoever drives it — __call__ for a solo call, _call_batched for each image of a batched one:
          ("fwd",)                           the guidance forward nothing consumes (an unguided image)
          ("eval", nxt) -> loss parts        one guidance evaluation; `nxt` (the refinement loop's evaluations; else None) is
                                             the request that follows if the loss is not zero, for a driver that enqueues ahead
          ("update", step, loss) -> mean |grad|   latents - step * dloss/dlatents of the evaluation just read
          ("momentum", lr, first, loss)      the `use_optimizer` step on that gradient
          ("joint",) -> loss parts           guidance evaluation + CFG pair as one batch-3 pass, the CFG + DDIM step included
          ("cfg",)                           CFG pass + DDIM step
          ("renoise", a, b)                  latents <- a * latents + b * noise
        `joint`: the driver serves ("joint",).  The image's guidance state is what shared_state holds while it runs."""
        hp = state.curHyperParams
        recurse_steps, recurse_until = max(hp.get("recurse_steps", 1), 1), hp.get("recurse_until", 20)
        guided = bool(getattr(state.config, "token_dict", None)) or bool(getattr(state.config, "custom_loss", None))
        for recurse_step in range(recurse_steps):
            did_we_update = False
            helpers.log(f"iteration {i}", self.verbose)
            may_update = (not state.config.only_update_on_threshold_steps and i < max_iter_to_alter) or \
                         (i in state.config.thresholds) or (i in thresholds)
            joint_step = guided and joint and not may_update and not run_standard_sd and not self.skip_unused_guidance
            if not guided:
                # nothing to guide (no annotated token): the reference still runs the guidance forward here,
                # with no consumer; kept only for call-count fidelity unless skip_unused_guidance is set
                if not self.skip_unused_guidance:
                    self.unet_calls["fwd_b1_grad"] += 1
                    yield ("fwd",)
            elif joint_step:
                # The guidance evaluation of this step cannot change the latents (no threshold, no per-step update): its
                # forward and the CFG pair see the SAME latents and run as one batch-3 pass.  Every evaluation of the
                # reference is still performed.  The loss of such a step is only logged: the device values are kept and read
                # back at the end of the call (no host sync here, the host runs ahead of the GPU); _flush_image_logs puts the
                # log lines in their place
                self.unet_calls["fwd_b1_grad"] += 1
                self.unet_calls["joint_b3"] += 1  # of fwd_b1_grad and fwd_b2, how many ran as one batch-3 pass
                parts = yield ("joint",)
                self._deferred_losses.append((len(helpers.lines), i, parts))
            elif not (self.skip_unused_guidance and (run_standard_sd or not may_update)):
                self.unet_calls["fwd_b1_grad"] += 1
                losses_dict = self._loss_host(*(yield ("eval", None)))
                if not run_standard_sd:
                    loss, losses, unscaled_losses = self._compute_loss(losses_dict=losses_dict)
                    if not self.meets_threshold(i, thresholds, unscaled_losses):
                        did_we_update = True
                        losses_dict = yield from self._perform_iterative_refinement_step(step_size, 10)
                    if (not state.config.only_update_on_threshold_steps and i < max_iter_to_alter) or \
                            (i in state.config.thresholds):
                        # the reference tests the losses from BEFORE the refinement here (:999)
                        if not self.meets_threshold(-1, state.config.thresholds, unscaled_losses):
                            did_we_update = True
                            loss, losses, unscaled_losses = self._compute_loss(losses_dict=losses_dict)
                            if losses_dict["_fused"]["host_total"].item() != 0:  # :1002
                                yield from self._request_update(("update", step_size, loss))
                        helpers.log(f"Iteration {i} | Loss: {losses_dict['_fused']['host_total'].item():0.4f}", self.verbose)
            self.unet_calls["fwd_b2"] += 1
            if not joint_step:
                yield ("cfg",)
            if i > recurse_until or not did_we_update:
                break
            if recurse_step != recurse_steps - 1:
                # back to the noise level of step t (reference :1047-1053)
                prev_timestep = t_int - self.scheduler.config.num_train_timesteps // self.scheduler.num_inference_steps
                if prev_timestep > 0:
                    Bt = self.scheduler.alphas_for(t_int)[0] / float(self.scheduler.alphas_cumprod[prev_timestep])
                    yield ("renoise", math.sqrt(Bt), math.sqrt(1 - Bt))

    def _perform_iterative_refinement_step(self, step_size, max_refinement_steps):
        """Update the latents until every sub-prompt meets the step's threshold or the iteration cap is hit (reference
        :475-581), then one more evaluation, whose losses_dict is returned and whose graph the step differentiates."""
        self.inside_iterative_refinement = True
        iteration = 0
        state.sub_iteration = iteration
        unscaled_losses = None
        # reference :495-497: SGD([latents], lr=step_size / 2.5, momentum=0.8), new for every refinement call — the call's
        # first step does not read the velocity
        momentum, first = bool(state.curHyperParams.get("use_optimizer", False)), True
        while unscaled_losses is None or not self.meets_threshold(state.cur_time_step_iter, state.config.thresholds,
                                                                  unscaled_losses):
            helpers.log(f"subiteration: {iteration}")
            iteration += 1
            state.sub_iteration = iteration
            update = ("momentum", float(step_size) / 2.5, first) if momentum else ("update", step_size)
            self.unet_calls["fwd_b1_grad"] += 1
            losses_dict = self._loss_host(*(yield ("eval", update)))
            loss, losses, unscaled_losses = self._compute_loss(losses_dict, return_losses=True)
            # reference :549-551: `loss.backward(); optim.step()` on any loss, `elif loss != 0` for the plain update
            if momentum or not self._loss_is_zero(losses_dict):
                yield from self._request_update(update + (loss,))
                first = False
            if iteration >= max_refinement_steps:
                helpers.log(f"\t Exceeded max number of iterations ({max_refinement_steps})! ", self.verbose)
                break
        self.unet_calls["fwd_b1_grad"] += 1
        final = self._loss_host(*(yield ("eval", None)))
        self._compute_loss(final, return_losses=True)
        helpers.log(f"\t Finished with loss of: {final['_fused']['host_total'].item()} iter: {iteration}", self.verbose)
        state.sub_iteration = 0
        return final

    def _request_update(self, request):
        """One backward pass and the latent update `request` names; the plain update's mean |grad| is logged at the end of
        the call (a device scalar until then).  The momentum step has no such line (reference :549-551)."""
        self.unet_calls["bwd"] += 1
        absmean = yield request
        if request[0] == "update":
            self._deferred_log.append(("gradient size average: ", absmean))

    def _resume(self, im, prog, reply, i):
        """Run an image's program up to its next request (-> the request; None: the step is done), with the image's own log,
        counters, sub-iteration and guidance state (shared_state.config / curHyperParams) in the places the program and the
        loss path read them."""
        saved = helpers.lines, self.unet_calls, self._deferred_log, self._deferred_losses, state.config, state.curHyperParams
        helpers.lines, self.unet_calls = im.lines, im.calls
        self._deferred_log, self._deferred_losses = im.deferred_log, im.deferred_losses
        state.config, state.curHyperParams = im.cfg, im.hp
        state.cur_time_step_iter, state.sub_iteration = i, im.sub_iteration
        try:
            return prog.send(reply)
        except StopIteration:
            return None
        finally:
            im.sub_iteration = state.sub_iteration
            (helpers.lines, self.unet_calls, self._deferred_log, self._deferred_losses, state.config,
             state.curHyperParams) = saved

    def _flush_image_logs(self, im):
        """The end of a call for one image: its deferred gradient sizes, then the loss lines of its log-only (joint) steps
        inserted where they belong.  Device values are read in ONE device -> host copy each."""
        saved = helpers.lines, self.unet_calls, state.config, state.curHyperParams
        helpers.lines, self.unet_calls = im.lines, im.calls
        state.config, state.curHyperParams = im.cfg, im.hp
        try:
            if im.deferred_log:
                vals = torch.stack([v.detach().reshape(()).float() for _, v in im.deferred_log]).cpu()
                for (text, _), v in zip(im.deferred_log, vals):
                    helpers.log(text + str(v.item()))
            if im.deferred_losses:   # the packed loss tables of one image: same plan, same length
                host_rows = torch.stack([parts[4] for _, _, parts in im.deferred_losses]).cpu()
            shift = 0
            for j, (pos, step, parts) in enumerate(im.deferred_losses):
                state.cur_time_step_iter, state.sub_iteration = step, 0
                mark = len(helpers.lines)
                self._compute_loss(losses_dict=self._loss_host(*parts[:4], host_rows[j]))
                fresh = helpers.lines[mark:]
                del helpers.lines[mark:]
                helpers.lines[pos + shift:pos + shift] = fresh
                shift += len(fresh)
            del im.deferred_log[:], im.deferred_losses[:]
        finally:
            helpers.lines, self.unet_calls, state.config, state.curHyperParams = saved

    discarded_speculations = 0   # evaluations enqueued ahead of a `loss != 0` test that came out the other way (never counted)
    verbose = False

    # ------------------------------------------------------------------ the denoising loop
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None], attention_store: AttentionStore, attention_res: int = 16,
                 height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                 guidance_scale: float = 7.5, negative_prompt: Optional[Union[str, List[str]]] = None,
                 num_images_per_prompt: Optional[int] = 1, eta: float = 0.0,
                 generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 output_type: Optional[str] = "pil", return_dict: bool = True,
                 callback: Optional[Callable[[int, int, torch.Tensor], None]] = None, callback_steps: int = 1,
                 cross_attention_kwargs: Optional[Dict[str, Any]] = None, max_iter_to_alter: Optional[int] = 25,
                 run_standard_sd: bool = False, thresholds: Optional[dict] = {0: 0.05, 10: 0.5, 20: 0.8},
                 scale_factor: int = 20, scale_range: Tuple[float, float] = (1., 0.5), smooth_attentions: bool = True,
                 sigma: float = 0.5, kernel_size: int = 3, sd_2_1: bool = False,
                 renoise_noise: Optional[List[torch.Tensor]] = None,
                 guidance_states: Optional[List["GuidanceState"]] = None,
                 variance_noise: Optional[List[torch.Tensor]] = None):
        """Same keywords as the reference (:747-777).  Extra, optional: `renoise_noise`, a list of host-generated
        noise tensors consumed by the recurse re-noise step instead of the device generator (RNG parity runs);
        `output_type="latent"` returns the final latents without the VAE.

        `eta` (0 <= eta <= 1) goes to every CFG + DDIM step, as the reference hands it to its scheduler (:906).  With eta > 0
        each CFG step consumes one standard-normal tensor of the latents' shape: the next one of `variance_noise` (a list of
        host tensors, one per CFG step in call order — recurse rounds make more CFG steps than timesteps; a batched call takes
        a list of S such lists), or, without it, a torch.randn draw from the call's `generator`, the one prepare_latents drew
        from (a batched call: generator[s] for image s).  The re-noise generator is not touched.  Ignored at eta = 0.

        `guidance_states` (one GuidanceState per prompt): guide P different prompts — `prompt` a list of P strings, or
        `prompt_embeds` / `negative_prompt_embeds` of P rows — each with its own annotation layout, threshold table and
        hyper-parameters, num_images_per_prompt = N images of each, S = P * N <= 64 images in prompt-major order (image s
        belongs to prompt s // N) in shared batched passes.  Image s does what a solo call does with
        shared_state.config = guidance_states[s // N].config, shared_state.curHyperParams = its hyper_params, prompt s // N
        and generator s: the same counters and log lines.  It needs a list of S generators or `latents` (S, 4, h, w);
        `renoise_noise` is a list of S per-image lists; `negative_prompt` None or a list of P.  Image s's threshold table is
        its config.thresholds (what run.run_on_prompt passes as `thresholds=`): the call's `thresholds` keyword is NOT read
        in this form.  A state without box or coordinate tokens rides along unguided."""
        eta = float(eta)
        if not 0.0 <= eta <= 1.0:   # before the device check and before any launch; a NaN fails the comparison
            raise ValueError(f"eta = {eta}: the DDIM step serves 0 <= eta <= 1")
        # a prediction type the DDIM step does not serve is refused here: before the device check and before any launch
        ops.prediction_code(getattr(self.scheduler.config, "prediction_type", "epsilon"))
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps, negative_prompt, prompt_embeds, negative_prompt_embeds)
        self.prompt = prompt
        batch_size = 1 if isinstance(prompt, str) else (len(prompt) if prompt is not None else prompt_embeds.shape[0])
        if guidance_states is not None:
            per_prompt = int(num_images_per_prompt or 1)
            states = self._check_states(guidance_states, batch_size, per_prompt, negative_prompt, guidance_scale, generator,
                                        latents, renoise_noise)
            self._check_variance_inputs(batch_size * per_prompt, eta, generator, variance_noise, "a call with guidance_states")
            if self.device.type != "cuda":
                raise GaError("GuidedAttention runs on the GPU only (HIP kernels); there is no CPU fallback")
            return self._call_batched(batch_size * per_prompt, prompt, attention_store, attention_res, height, width,
                                      num_inference_steps, guidance_scale, negative_prompt, generator, latents, prompt_embeds,
                                      negative_prompt_embeds, output_type, return_dict, callback, callback_steps,
                                      max_iter_to_alter, run_standard_sd, thresholds, scale_factor, scale_range,
                                      smooth_attentions, sigma, kernel_size, sd_2_1, renoise_noise, states=states, eta=eta,
                                      variance_noise=variance_noise)
        if batch_size != 1:
            raise NotImplementedError("a list of different prompts: the guidance pass serves one prompt (the reference "
                                      "indexes prompt_embeds[1]); several images of it: num_images_per_prompt")
        images = int(num_images_per_prompt or 1)
        if images > 1:
            self._check_batched(images, generator, latents, renoise_noise)
            self._check_variance_inputs(images, eta, generator, variance_noise, "num_images_per_prompt > 1")
        device = self.device
        if device.type != "cuda":
            raise GaError("GuidedAttention runs on the GPU only (HIP kernels); there is no CPU fallback")
        if images > 1:
            return self._call_batched(images, prompt, attention_store, attention_res, height, width, num_inference_steps,
                                      guidance_scale, negative_prompt, generator, latents, prompt_embeds,
                                      negative_prompt_embeds, output_type, return_dict, callback, callback_steps,
                                      max_iter_to_alter, run_standard_sd, thresholds, scale_factor, scale_range,
                                      smooth_attentions, sigma, kernel_size, sd_2_1, renoise_noise, eta=eta,
                                      variance_noise=variance_noise)
        do_cfg = guidance_scale > 1.0
        _, prompt_embeds = self._encode_prompt(prompt, device, num_images_per_prompt, do_cfg, negative_prompt,
                                               prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds)
        prediction, timesteps, scale_range, max_iter_to_alter = self._begin_call(
            num_inference_steps, scale_range, max_iter_to_alter, attention_store, attention_res, height, width)
        latents = self.prepare_latents(1, self.unet.in_channels, height, width, prompt_embeds.dtype, device, generator,
                                       latents)
        im = self._image_record(state.config, state.curHyperParams, thresholds, helpers.lines, generator, renoise_noise,
                                variance_noise, eta)
        self.unet_calls, self._deferred_log, self._deferred_losses = im.calls, im.deferred_log, im.deferred_losses
        cond = prompt_embeds[1:2] if do_cfg else prompt_embeds[0:1]
        self._runner = None
        self._dump = bool(self.reference_side_effects or getattr(state.config, "diagnostic_level", 0) > 0)
        # paint-with-words changes the attention kernels' arguments from step to step (sigma_t, on / off): eager
        paint = bool((state.curHyperParams or {}).get("paint_with_words_stop", 0))
        custom = getattr(state.config, "custom_loss", None)
        if im.guided and self._relations_eligible(custom):
            # the relation rows: resolved, validated and uploaded before the first launch and before any capture
            self._solo_relation_table(attention_res, smooth_attentions, sigma, kernel_size,
                                      self._last_text_index(prompt_embeds.shape[1], sd_2_1))
        if self.use_graphs and do_cfg and im.guided and not run_standard_sd and not self._dump and not paint:
            from .graphs import GraphRunner
            self._runner = GraphRunner.for_run(self, attention_store, prompt_embeds, latents, attention_res,
                                               smooth_attentions, sigma, kernel_size, sd_2_1)
        runner = self._runner
        ev_args = (attention_store, attention_res, smooth_attentions, sigma, kernel_size, sd_2_1)
        # Run-ahead, inside the iterative refinement on the runner: an evaluation's backward, latent update and the NEXT
        # evaluation are enqueued before the evaluation is answered, i.e. before the program's _loss_host waits for its table
        # (PendingLossTable: for that table only).  The GPU runs eval -> backward -> update -> eval ... back to back; the
        # device -> host copy of each table and the host's threshold logic overlap the next pass (215 us + 129 us of idle GPU
        # per iteration otherwise, profiles/r3_gpu_idle_gaps.md).  Same launches in the same order as reading first: what is
        # assumed is `loss != 0` (reference :551), and a loss of exactly 0 drops what was enqueued ahead, uncounted.
        run_ahead = (runner is not None and self.speculative_refinement and not custom
                     and self._loss_plan(smooth_attentions, sigma, kernel_size).T > 0)
        velocity = None   # `use_optimizer`: one f32 buffer for the call; the first step of a refinement call does not read it
        if state.curHyperParams.get("use_optimizer", False):
            velocity = torch.empty(latents.shape, dtype=torch.float32, device=device)

        def step_latents(request, loss):
            """The backward pass of `loss` and the update `request` names -> (new latents, mean |grad| of a plain update)"""
            grad = self._latent_gradient(leaf, loss)
            if request[0] == "momentum":
                return ops.latent_sgd_momentum(leaf.detach(), grad, velocity, request[1], 0.8, request[2]), None
            return ops.latent_axpy(leaf.detach(), grad, float(request[1]), True)

        def resume(reply):
            with torch.enable_grad():   # a plugin's loss is added to the built-in one inside the program (_compute_loss)
                return self._resume(im, prog, reply, i)

        for i, t in enumerate(timesteps):
            t_int = int(t)
            a_t, a_prev = self.scheduler.alphas_for(t_int)
            prog = self._guidance_step(i, t_int, im.thresholds, scale_factor * np.sqrt(scale_range[i]), max_iter_to_alter,
                                       run_standard_sd, runner is not None and runner.joint)
            # leaf: what the last evaluation's loss depends on (the runner's ONE static buffer, or a clone); `latents` is
            # never that buffer, so an evaluation enqueued ahead starts from a tensor of its own.  ahead: an evaluation
            # enqueued before it was asked for; stepped: the update enqueued before it, until the program asks for it
            leaf = ahead = stepped = None
            request = resume(None)
            while request is not None:
                kind, reply = request[0], None
                if kind == "eval":
                    if stepped is not None:   # the loss was exactly 0: no update (reference :551), the unchanged latents again
                        self.discarded_speculations += 1
                        ahead = stepped = None
                    leaf, reply = ahead or self._guidance_parts(latents, t_int, cond, *ev_args)
                    ahead = None
                    if run_ahead and request[1] is not None:
                        stepped = step_latents(request[1], runner.loss)
                        ahead = runner.evaluate(stepped[0], t_int, attention_store)
                elif kind in ("update", "momentum"):
                    with torch.enable_grad():
                        latents, reply = stepped or step_latents(request, request[-1])
                    stepped = None
                elif kind == "fwd":
                    self._guidance_forward(latents, t_int, cond)
                elif kind == "renoise":
                    latents = ops.latent_axpby(latents, self._renoise_draw(im, latents), request[1], request[2])
                else:   # "joint", "cfg": the noise prediction, the fused CFG combine + DDIM step and the per-round side work
                    if kind == "joint":
                        parts, noise_pred = runner.joint_forward(latents, t_int, attention_store)
                        reply = parts[:4] + (parts[4].clone(),)   # the next replay overwrites the static row
                    elif runner is not None:
                        noise_pred = runner.cfg_forward(latents, t_int, attention_store)
                    else:
                        model_in = self.scheduler.scale_model_input(torch.cat([latents] * 2) if do_cfg else latents, t_int)
                        noise_pred = self.unet(model_in, t_int, encoder_hidden_states=prompt_embeds).sample
                    z = None
                    if eta > 0.0:
                        z = draw_variance_noise(im.variance_src, latents.shape, latents.dtype, device,
                                                f"image 0, CFG step {im.variance_draws}")
                        im.variance_draws += 1
                    eps_uncond, eps_text = noise_pred.chunk(2) if do_cfg else (noise_pred, noise_pred)
                    latents, _x0 = ops.cfg_ddim_step(eps_uncond, eps_text, guidance_scale if do_cfg else 1.0, latents, a_t,
                                                     a_prev, self._dump, prediction, eta, z)
                    if self._dump:  # reference :1031-1037 (each of these synchronises with the device)
                        helpers.log_latent_stats(latents, True)
                        if state.config.diagnostic_level > 1:
                            self.save_image(latents, "xt")
                        if (state.config.diagnostic_level > 0 or state.cur_time_step_iter in state.always_save_iter) \
                                and self.vae is not None:
                            self.save_image(_x0, "pred")
                    if callback is not None and i % callback_steps == 0:
                        callback(i, t_int, latents)
                request = resume(reply)
        self._flush_image_logs(im)
        return self._finish_call(latents, output_type, return_dict, unet_calls=dict(self.unet_calls),
                                 variance_draws=im.variance_draws)

    def _begin_call(self, num_inference_steps, scale_range, max_iter_to_alter, attention_store, attention_res, height, width):
        """What a solo and a batched call set up alike: a fresh scheduler with the call's timesteps, the shared_state values
        the loss path and the diagnostics read, the per-step scale of the update.  -> (prediction type of every CFG + DDIM
        launch of the call, timesteps, scale_range per step, max_iter_to_alter)."""
        state.always_save_iter = [0, 1, 2]
        self.scheduler = DDIMScheduler.from_config(self.scheduler.config)
        self.scheduler.set_timesteps(num_inference_steps, device="cpu")
        timesteps = self.scheduler.timesteps
        acp = self.scheduler.alphas_cumprod
        state.sigmas = (((1 - acp) / acp) ** 0.5).numpy()
        state.timesteps = timesteps
        if max_iter_to_alter is None:
            max_iter_to_alter = len(timesteps) + 1
        if hasattr(attention_store, "attention_res"):
            attention_store.attention_res = attention_res
        self._attention_store = attention_store
        self._truncate_at = self._truncation_point(attention_res, height, width)
        return (self.scheduler.config.prediction_type, timesteps, np.linspace(scale_range[0], scale_range[1], len(timesteps)),
                max_iter_to_alter)

    def _image_record(self, cfg, hp, thresholds, lines, generator, renoise_noise, variance_noise, eta):
        """What one image of a call carries from step to step: its log, call counters and deferred log entries, its guidance
        state and threshold table (what _resume installs while its program runs), its noise sources.  The re-noise source is
        the image's list, else a generator seeded like the image's own (deterministic recurse, reference :921); the variance
        source (eta > 0) is its list, else the generator its latents came from."""
        noise = list(renoise_noise) if renoise_noise is not None else None
        if noise is None and max(hp.get("recurse_steps", 1), 1) > 1:
            noise = torch.Generator(self.device).manual_seed(generator.initial_seed() if generator is not None else 0)
        variance_src = None   # eta = 0: `variance_noise` is not looked at
        if eta > 0.0:
            variance_src = list(variance_noise) if variance_noise is not None else generator
        return SimpleNamespace(lines=lines, deferred_log=[], deferred_losses=[], sub_iteration=0, noise=noise,
                               variance_src=variance_src, variance_draws=0,
                               calls={"fwd_b1_grad": 0, "bwd": 0, "fwd_b2": 0, "loss_evals": 0, "joint_b3": 0},
                               cfg=cfg, hp=hp, thresholds=thresholds if len(thresholds) else {0: float("inf")},
                               guided=bool(getattr(cfg, "token_dict", None)) or bool(getattr(cfg, "custom_loss", None)))

    def _renoise_draw(self, im, latents):
        """The next re-noise tensor of image `im`, of the shape and dtype of its `latents`."""
        if isinstance(im.noise, list):
            return im.noise.pop(0).to(device=latents.device, dtype=latents.dtype)
        return torch.randn(latents.shape, generator=im.noise, device=latents.device).to(latents.dtype)

    def _finish_call(self, latents, output_type, return_dict, **fields):
        """latents -> decoded images (numpy, or PIL) unless output_type is "latent"; the call's return value."""
        image = latents
        if output_type != "latent":
            image = self.decode_latents(latents)
            if output_type == "pil":
                image = self.numpy_to_pil(image)
        if not return_dict:
            return (image, False)
        return PipelineOutput(images=image, nsfw_content_detected=False, latents=latents, **fields)

    # ------------------------------------------------------------------ S images per call (num_images_per_prompt > 1)
    def _check_batched(self, images, generator, latents, renoise_noise):
        """Requests the batched path does not serve: raised before any GPU launch (and before the device check)."""
        from ._lib import GA_MAX_IMAGES
        if images > GA_MAX_IMAGES:
            raise ValueError(f"num_images_per_prompt = {images}: at most {GA_MAX_IMAGES} images per call")
        for hit, what in self._refused_in_batched(state.config, state.curHyperParams or {}):
            if hit:
                raise NotImplementedError(f"{what} with num_images_per_prompt > 1 is not supported")
        self._check_relations(state.config)
        self._check_image_inputs(images, generator, latents, renoise_noise, "num_images_per_prompt > 1",
                                 "num_images_per_prompt is")

    def _refused_in_batched(self, cfg, hp):
        """(asked for, its name) of everything a call with several images does not serve, for one guidance state"""
        custom = getattr(cfg, "custom_loss", None)
        return [(bool(custom) and not self._relations_eligible(custom), "custom-loss plugins"),
                (bool(hp.get("paint_with_words_stop", 0)) and not self.batched_paint_with_words, "paint-with-words"),
                (bool(self.reference_side_effects), "reference_side_effects"),
                (getattr(cfg, "diagnostic_level", 0) > 0, "diagnostic_level > 0"),
                (not self.fused_aggregate_loss, "fused_aggregate_loss = False"),
                (bool(hp.get("use_optimizer", False)) and not self.batched_momentum_refinement, "use_optimizer"),
                (self.unet.config.addition_embed_type is not None, "a UNet with added conditioning (SDXL layout)")]

    @staticmethod
    def _check_image_inputs(images, generator, latents, renoise_noise, form, count):
        if isinstance(generator, torch.Generator):
            raise ValueError(f"{form} needs a list of one generator per image (or `latents`): with one "
                             "generator no solo call would reproduce image s > 0")
        if generator is not None and len(generator) != images:
            raise ValueError(f"{len(generator)} generators for {images} images")
        if latents is None and generator is None:
            raise ValueError(f"{form} needs a list of generators or `latents` of shape (S, 4, h, w)")
        if latents is not None and latents.shape[0] != images:
            raise ValueError(f"latents hold {latents.shape[0]} images, {count} {images}")
        if renoise_noise is not None and len(renoise_noise) != images:
            raise ValueError(f"renoise_noise must be a list of {images} per-image lists")

    @staticmethod
    def _check_variance_inputs(images, eta, generator, variance_noise, form):
        """eta > 0 in a batched call: image s draws its variance noise from generator s or takes it from variance_noise[s]; with
        neither, no solo call would reproduce an image (the rule of _check_image_inputs).  Raised before any launch."""
        if eta == 0.0:
            return
        if variance_noise is not None:
            if len(variance_noise) != images or not all(isinstance(v, (list, tuple)) for v in variance_noise):
                raise ValueError(f"variance_noise must be a list of {images} per-image lists")
        elif generator is None:
            raise ValueError(f"{form} with eta > 0 needs a list of generators or `variance_noise` (one list per image)")

    def _check_states(self, guidance_states, prompts, per_prompt, negative_prompt, guidance_scale, generator, latents,
                      renoise_noise):
        """A call with guidance_states: what it does not serve is raised before any GPU launch (and before the device check),
        per state, naming the prompt."""
        from ._lib import GA_MAX_IMAGES
        states = list(guidance_states)
        if len(states) != prompts:
            raise ValueError(f"{len(states)} guidance_states for {prompts} prompts: one state per prompt")
        images = prompts * per_prompt
        if not 1 <= images <= GA_MAX_IMAGES:
            raise ValueError(f"{prompts} prompts x {per_prompt} images = {images}: at most {GA_MAX_IMAGES} images per call")
        if negative_prompt is not None and (isinstance(negative_prompt, str) or len(negative_prompt) != prompts):
            raise ValueError(f"negative_prompt must be None or a list of {prompts} (one per prompt)")
        for p, st in enumerate(states):
            if not isinstance(st, GuidanceState):
                raise ValueError(f"guidance_states[{p}] is not a GuidanceState")
            refused = self._refused_in_batched(st.config, st.hyper_params or {}) + \
                [(not guidance_scale > 1.0, "guidance_scale <= 1 (no classifier-free-guidance pass)")]
            for hit, what in refused:
                if hit:
                    raise NotImplementedError(f"prompt {p}: {what} is not supported in a call with guidance_states")
            self._check_relations(st.config)
        self._check_image_inputs(images, generator, latents, renoise_noise, "a call with guidance_states", "the call guides")
        return states

    def _call_batched(self, S, prompt, attention_store, attention_res, height, width, num_inference_steps, guidance_scale,
                      negative_prompt, generator, latents, prompt_embeds, negative_prompt_embeds, output_type,
                      return_dict, callback, callback_steps, max_iter_to_alter, run_standard_sd, thresholds, scale_factor,
                      scale_range, smooth_attentions, sigma, kernel_size, sd_2_1, renoise_noise, states=None, eta=0.0,
                      variance_noise=None):
        """S images of one prompt, or (`states`: one GuidanceState per prompt) of P prompts in prompt-major order, each
        guided by its own state.  Each image runs the step program (_guidance_step) a solo call runs, one of its own; the
        driver below batches what the programs ask for into passes of batch S — images outside a pass are idle slots —
        and answers them with the masked launches, so that image s does exactly what a solo call on its inputs does.  One difference: `callback`
        is called once per denoising step, with the (S, 4, h, w) latents after every image has finished the step (a solo
        call calls it after each of its CFG steps, i.e. once per recurse round); images finish their recurse rounds at
        different passes, so no per-round latents of all S images exist."""
        device = self.device
        do_cfg = guidance_scale > 1.0
        if not do_cfg:
            raise NotImplementedError("num_images_per_prompt > 1 runs the classifier-free-guidance pass (guidance_scale > 1)")
        P = len(states) if states is not None else 1
        N = S // P
        _, prompt_embeds = self._encode_prompt(prompt, device, N, do_cfg, negative_prompt, prompt_embeds=prompt_embeds,
                                               negative_prompt_embeds=negative_prompt_embeds)   # [uncond x S; cond x S]
        prediction, timesteps, scale_range, max_iter_to_alter = self._begin_call(
            num_inference_steps, scale_range, max_iter_to_alter, attention_store, attention_res, height, width)
        if latents is None:   # image s: what the solo call's prepare_latents draws from generator s
            latents = torch.cat([self.prepare_latents(1, self.unet.in_channels, height, width, prompt_embeds.dtype, device,
                                                      g) for g in generator])
        else:
            latents = torch.cat([self.prepare_latents(1, self.unet.in_channels, height, width, prompt_embeds.dtype, device,
                                                      None, latents[s:s + 1]) for s in range(S)])
        imgs = []
        for s in range(S):
            # image s's guidance state: its prompt's GuidanceState, or the shared_state globals of a one-prompt call; the
            # threshold table is what the solo call gets as `thresholds` (run.run_on_prompt passes config.thresholds); its
            # noise sources are the solo call's (generator s, list s)
            cfg, hp = (states[s // N].config, states[s // N].hyper_params) if states is not None else \
                (state.config, state.curHyperParams)
            imgs.append(self._image_record(cfg, hp, dict(cfg.thresholds) if states is not None else thresholds, [],
                                           generator[s] if generator is not None else None,
                                           renoise_noise[s] if renoise_noise is not None else None,
                                           variance_noise[s] if eta > 0.0 and variance_noise is not None else None, eta))
        cond = prompt_embeds[S:]
        guided = any(im.guided for im in imgs)
        self._dump = False
        self._images = S
        # one descriptor row per image: images of different states, and any call with a relation (the relation launches take rows)
        if guided and (states is not None or any(getattr(im.cfg, "custom_loss", None) for im in imgs)):
            self._table = self._image_table(imgs, prompt, prompt_embeds.shape[1], attention_res, smooth_attentions, sigma,
                                            kernel_size, sd_2_1, N)
        passes = {"eval": 0, "bwd": 0, "cfg": 0, "joint": 0, "idle_slots": 0}

        def variance_noise_for(who, latents):
            """The packed (S, 4, h, w) variance noise of one masked CFG + DDIM step: each image of the pass consumes one tensor of
            its own source, an idle slot consumes nothing and gets zeros (the launch drops its slice).  None at eta = 0."""
            if eta == 0.0:
                return None
            z = torch.zeros_like(latents)
            for s in who:
                im = imgs[s]
                z[s:s + 1] = draw_variance_noise(im.variance_src, latents[s:s + 1].shape, latents.dtype, device,
                                                 f"image {s}, CFG step {im.variance_draws}")
                im.variance_draws += 1
            return z
        outer_lines = helpers.lines
        # paint-with-words changes the attention kernels' arguments from step to step (sigma_t, on / off per image): if any image
        # of the call paints, the whole call is eager — no runner, hence no joint passes — as a solo paint-with-words call is
        paint = any(bool((im.hp or {}).get("paint_with_words_stop", 0)) for im in imgs)
        # `use_optimizer` images: one f32 velocity slice per image for the whole call, never cleared — the first step of each of an
        # image's refinement calls does not read its slice (the program's `first`)
        velocity = None
        if any(bool((im.hp or {}).get("use_optimizer", False)) for im in imgs):
            velocity = torch.empty(latents.shape, dtype=torch.float32, device=device)
        try:
            self._runner = None
            if self.use_graphs and guided and not run_standard_sd and not paint:
                from .graphs import GraphRunner
                self._runner = GraphRunner.for_run(self, attention_store, prompt_embeds, latents, attention_res,
                                                   smooth_attentions, sigma, kernel_size, sd_2_1)
            runner = self._runner
            ev_args = (attention_store, attention_res, smooth_attentions, sigma, kernel_size, sd_2_1)
            for i, t in enumerate(timesteps):
                t_int = int(t)
                a_t, a_prev = self.scheduler.alphas_for(t_int)
                if paint:   # one record per image for every pass of step i: its state and its multiplier (0 past its stop)
                    ptp_utils.set_paint_images(SimpleNamespace(config=im.cfg, hp=im.hp, mult=ptp_utils.paint_multiplier(im.hp, i))
                                               for im in imgs)
                # per image: its own threshold steps, update policy and recurse settings, read from its state as it runs
                progs = [self._guidance_step(i, t_int, im.thresholds, scale_factor * np.sqrt(scale_range[i]), max_iter_to_alter,
                                             run_standard_sd, runner is not None and runner.joint) for im in imgs]
                pending = {s: self._resume(imgs[s], progs[s], None, i) for s in range(S)}
                pending = {s: r for s, r in pending.items() if r is not None}
                leaf = loss_vec = None
                while pending:
                    kinds = {r[0] for r in pending.values()}
                    kind = next(k for k in ("update", "momentum", "eval", "fwd", "joint", "cfg", "renoise") if k in kinds)
                    if kind == "momentum":   # plain and momentum updates of one evaluation are ONE backward pass
                        kind = "update"
                    who = sorted(s for s, r in pending.items() if r[0] == kind or (kind == "update" and r[0] == "momentum"))
                    active = [int(s in who) for s in range(S)]
                    replies = {}
                    if kind in ("eval", "update", "cfg", "joint"):
                        passes["bwd" if kind == "update" else kind] += 1
                        passes["idle_slots"] += S - len(who)
                    if kind == "update":   # the backward of the evaluation just read, BEFORE the next evaluation replaces it
                        mask = ops._device_vector([float(a) for a in active], torch.float32, device)
                        plain = [s for s in who if pending[s][0] == "update"]
                        stepping = [s for s in who if pending[s][0] == "momentum"]
                        if runner is not None:
                            runner.grad_mask.copy_(mask)
                            grad = runner.backward()
                        else:
                            grad = torch.autograd.grad(loss_vec, [leaf], grad_outputs=[mask], retain_graph=True)[0]
                            ops.end_image_broadcasts()
                        latents = leaf.detach()
                        if plain:
                            steps = [float(pending[s][1]) if s in plain else 0.0 for s in range(S)]
                            latents, absmean = ops.latent_axpy_batched(latents, grad, steps, [int(s in plain) for s in range(S)],
                                                                       True)
                            replies = {s: absmean[s] for s in plain}
                        if stepping:   # chained on the axpy's output: both launches pass the other set's images through bit for bit
                            lrs = [float(pending[s][1]) if s in stepping else 0.0 for s in range(S)]
                            firsts = [int(bool(pending[s][2])) if s in stepping else 0 for s in range(S)]
                            latents = ops.latent_sgd_momentum_batched(latents, grad, velocity, lrs, 0.8, firsts,
                                                                      [int(s in stepping) for s in range(S)])
                    elif kind == "eval":
                        leaf, parts = self._guidance_parts(latents, t_int, cond, *ev_args)
                        loss_vec = parts[1]
                        host = parts[4].cpu().reshape(S, -1)   # the S loss tables in ONE device -> host copy
                        replies = {s: self._image_parts(parts, s, host[s]) for s in who}
                    elif kind == "fwd":
                        self._guidance_forward(latents, t_int, cond)
                    elif kind == "joint":
                        parts, noise = runner.joint_forward(latents, t_int, attention_store)
                        packed = parts[4].reshape(S, -1).clone()
                        replies = {s: self._image_parts(parts, s, packed[s]) for s in who}
                        latents, _ = ops.cfg_ddim_step_masked(noise[:S], noise[S:], guidance_scale, latents, a_t, a_prev,
                                                              active, False, prediction, eta, variance_noise_for(who, latents))
                    elif kind == "cfg":
                        if runner is not None:
                            noise = runner.cfg_forward(latents, t_int, attention_store)
                        else:
                            model_in = self.scheduler.scale_model_input(torch.cat([latents] * 2), t_int)
                            noise = self.unet(model_in, t_int, encoder_hidden_states=prompt_embeds).sample
                        latents, _ = ops.cfg_ddim_step_masked(noise[:S], noise[S:], guidance_scale, latents, a_t, a_prev,
                                                              active, False, prediction, eta, variance_noise_for(who, latents))
                    else:   # renoise: back to the noise level of step t, each image from its own noise source
                        a, b = pending[who[0]][1], pending[who[0]][2]
                        noise = torch.zeros_like(latents)
                        for s in who:
                            noise[s:s + 1] = self._renoise_draw(imgs[s], latents[s:s + 1])
                        latents = ops.latent_axpby_masked(latents, noise, a, b, active)
                    for s in who:
                        pending[s] = self._resume(imgs[s], progs[s], replies.get(s), i)
                        if pending[s] is None:
                            del pending[s]
                if callback is not None and i % callback_steps == 0:
                    callback(i, t_int, latents)
            for im in imgs:
                self._flush_image_logs(im)
        finally:
            ptp_utils.set_paint_images(None)
            self._images = 1
            self._table = None
            helpers.lines = outer_lines
        per_image = [dict(im.calls) for im in imgs]
        self.unet_calls = {k: sum(c[k] for c in per_image) for k in per_image[0]}
        return self._finish_call(latents, output_type, return_dict, unet_calls=dict(self.unet_calls),
                                 unet_calls_per_image=per_image, batched_passes=passes, logs=[im.lines for im in imgs],
                                 variance_draws=[im.variance_draws for im in imgs])

    def _image_table(self, imgs, prompt, n_tok, attention_res, smooth, sigma, kernel_size, sd_2_1, per_prompt):
        """The descriptor rows of a call with guidance_states: image s's LossPlan (built from its own state, as its solo call
        builds it) and text slice — with sd_2_1 the slice ends at the EOT of image s's own prompt.  One ImageTable per
        (S, token capacity, call-level loss settings) is kept for the pipeline's lifetime: captured graphs read its buffer."""
        saved = state.config, state.curHyperParams
        plans, slices, rels = [], [], []
        try:
            for s, im in enumerate(imgs):
                state.config, state.curHyperParams = im.cfg, im.hp
                plans.append(self._loss_plan(smooth, sigma, kernel_size) if im.guided else
                             ops.LossPlan([], im.hp, smooth, sigma, kernel_size))
                rels.append(self._relation_plan())   # the image's own relation row (None: it has no custom loss)
                if sd_2_1:
                    text = prompt[s // per_prompt] if isinstance(prompt, list) else im.cfg.prompt
                    slices.append((1, len(self.tokenizer(text)["input_ids"]) - 1))
                else:
                    slices.append((1, n_tok - 1))
        finally:
            state.config, state.curHyperParams = saved
        T_max = ops.image_table_capacity(max(p.T for p in plans))
        Q_max = ops.relation_capacity(max(len(r.columns) if r is not None else 0 for r in rels))
        key = (len(imgs), T_max, attention_res, bool(smooth), float(sigma), int(kernel_size), str(self.device)) + \
            ((Q_max,) if Q_max else ())
        tables = self.__dict__.setdefault("_image_tables", {})
        if key not in tables:
            tables[key] = ops.ImageTable(len(imgs), T_max, attention_res, smooth, sigma, kernel_size, self.device, Q_max=Q_max)
        return tables[key].set(plans, slices, rels if Q_max else None)

    def _image_parts(self, parts, s, row):
        """Image s's loss parts from a batched evaluation (its terms, its loss, its plan, its packed row) in the form
        _loss_host takes for one image; a table call's rows are cut from T_max token rows down to the image's own T."""
        terms, loss, custom, plan, _ = parts
        if self._table is None:
            return terms[s], loss[s:s + 1], None, plan, row
        plan = self._table.plans[s]
        # an image with a relation row: the marker a solo call's parts carry (its packed pair is (box, relation) already)
        rel = FusedRelation(custom.value[s:s + 1]) if custom is not None and self._table.relations[s] is not None else None
        return terms[s, :plan.T], loss[s:s + 1], rel, plan, torch.cat([row[:plan.T * 8], row[-2:]])

    def _truncation_point(self, attention_res, height, width):
        """(up-block index, layers) after which no res^2 cross-attention map is produced any more."""
        lat = height // self.vae_scale_factor
        n_down = len(self.unet.down_blocks)
        last = None
        for i, blk in enumerate(self.unet.up_blocks):
            side = lat // (2 ** (n_down - 1 - i))
            if blk.has_cross_attention and side == attention_res:
                last = (i, len(blk.resnets))
        return last


GuidedAttentionPipeline = GuidedAttention  # the name the task framing uses
