#!/usr/bin/env python3
"""Images per second with S seeds guided in one batched call (num_images_per_prompt = S), on the workload of bench.py:
SD-1.x 512^2, fp16, the default guidance settings, hipGraph replay, the per-seed inputs of bench.make_run.  One process,
one JSON line per S:
images/s, ms per image, the device time of each pass kind at batch S (events around the replays), the per-image call
counters, the batched passes with their idle slots, and the peak memory.  The runner keeps one captured configuration and S
is part of it, so the S values are timed one after another (warm-up, timed calls, one call with events), not interleaved:
interleaving would time a graph capture in every call.

  python tools/seeds_per_pass_bench.py --seeds-per-pass 1,2,4 [--rounds 2] [--warmup 1]

--layouts K (K >= 1): every call guides its S images with K different box layouts and hyper-parameter states (a call with
guidance_states, image s on layout s % K; the JSON lines then carry "metric": "prompts_per_pass").  The graphs are captured in
the warm-up; each line records the graph captures of every timed call, which should all be 0.  Layout k moves the boxes of the
bench prompt and varies shrink_factor and the threshold table, so the images take different refinement counts.

  python tools/seeds_per_pass_bench.py --seeds-per-pass 2,4 --layouts 2

--use_optimizer: the same workload with `use_optimizer` in the hyper-parameters (SGD-momentum refinement; S > 1 through
GuidedAttention.batched_momentum_refinement).  The JSON lines carry "use_optimizer": true.

  python tools/seeds_per_pass_bench.py --seeds-per-pass 1,2,4 --use_optimizer"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


class PassTimer:
    """Device events around the GraphRunner's replays: ms per pass kind (sum over a call) and the number of replays."""

    KINDS = {"evaluate": "eval", "backward": "bwd", "cfg_forward": "cfg", "joint_forward": "joint"}

    def __init__(self):
        self.events = []

    def wrap(self, runner):
        for meth, kind in self.KINDS.items():
            fn = getattr(runner, meth)
            if getattr(fn, "_timed", False):
                continue

            def timed(*a, _fn=fn, _kind=kind, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = _fn(*a, **k)
                e1.record()
                self.events.append((_kind, e0, e1))
                return out
            timed._timed = True
            setattr(runner, meth, timed)

    def collect(self):
        torch.cuda.synchronize()
        ms, n = {}, {}
        for kind, e0, e1 in self.events:
            ms[kind] = ms.get(kind, 0.0) + e0.elapsed_time(e1)
            n[kind] = n.get(kind, 0) + 1
        self.events = []
        return {k: {"replays": n[k], "ms_total": round(ms[k], 3), "ms_per_pass": round(ms[k] / n[k], 4)} for k in ms}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds-per-pass", default="1,2,4")
    ap.add_argument("--rounds", type=int, default=2, help="timed calls per S")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="sd15", choices=["sd15", "tiny"])
    ap.add_argument("--layouts", type=int, default=0, help="K different layouts / hyper-parameter states per call (0: one prompt)")
    ap.add_argument("--use_optimizer", action="store_true", help="SGD-momentum refinement (batched_momentum_refinement at S > 1)")
    mine = ap.parse_args(argv)
    sizes = [int(x) for x in mine.seeds_per_pass.split(",")]
    args = bench.parse(["--model", mine.model])
    device = torch.device("cuda", 0)
    pipe, cfg, _ = bench.build_pipeline(args, device, 0, 1)
    pipe.speculative_refinement = True     # S = 1 keeps the run-ahead refinement of the headline; S > 1 does not use it
    one_image, rc, embeds = bench.make_run(args, pipe, cfg, device)
    from guided_attention_amd import ops
    from guided_attention_amd.graphs import GraphRunner
    from guided_attention_amd.utils import helpers, ptp_utils, shared_state as state
    if mine.use_optimizer:
        state.curHyperParams = dict(state.curHyperParams, use_optimizer=True)
        pipe.batched_momentum_refinement = True
    inputs = {S: [one_image.prepare(1000 + 97 * S + s) for s in range(S)] for S in sizes}
    states = [layout_state(k, rc, mine.use_optimizer) for k in range(mine.layouts)]

    def call(S):
        prepared = inputs[S]
        if mine.layouts:
            return call_layouts(S, prepared)
        if S == 1:
            return one_image(prepared[0])
        helpers.log_clear()
        state.cur_seed = prepared[0][0]
        controller = ptp_utils.AttentionStore()
        ptp_utils.register_attention_control(pipe, controller)
        return pipe(prompt=None, prompt_embeds=embeds[1:2], negative_prompt_embeds=embeds[0:1], attention_store=controller,
                    attention_res=rc.attention_res, guidance_scale=rc.guidance_scale,
                    num_inference_steps=rc.n_inference_steps, max_iter_to_alter=rc.max_iter_to_alter,
                    thresholds=rc.thresholds, scale_factor=rc.scale_factor, scale_range=rc.scale_range,
                    smooth_attentions=rc.smooth_attentions, sigma=rc.sigma, kernel_size=rc.kernel_size,
                    latents=torch.cat([p[1] for p in prepared]), renoise_noise=[list(p[2]) for p in prepared],
                    output_type="latent", num_images_per_prompt=S)

    def call_layouts(S, prepared):
        helpers.log_clear()
        state.cur_seed = prepared[0][0]
        controller = ptp_utils.AttentionStore()
        ptp_utils.register_attention_control(pipe, controller)
        return pipe(prompt=None, prompt_embeds=embeds[1:2].expand(S, -1, -1), negative_prompt_embeds=embeds[0:1].expand(S, -1, -1),
                    guidance_states=[states[s % mine.layouts] for s in range(S)], attention_store=controller,
                    attention_res=rc.attention_res, guidance_scale=rc.guidance_scale, num_inference_steps=rc.n_inference_steps,
                    max_iter_to_alter=rc.max_iter_to_alter, scale_factor=rc.scale_factor, scale_range=rc.scale_range,
                    smooth_attentions=rc.smooth_attentions, sigma=rc.sigma, kernel_size=rc.kernel_size,
                    latents=torch.cat([p[1] for p in prepared]), renoise_noise=[list(p[2]) for p in prepared],
                    output_type="latent")

    timer = PassTimer()
    stats = {S: {"seconds": 0.0, "images": 0, "passes": {}, "peak": 0, "captures": []} for S in sizes}
    last = {}
    for S in sizes:
        for _ in range(mine.warmup):   # captures the graphs at this S
            call(S)
        for _ in range(mine.rounds):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(device)
            captures = GraphRunner.captures
            t0 = time.perf_counter()
            out = call(S)
            torch.cuda.synchronize()
            stats[S]["seconds"] += time.perf_counter() - t0
            stats[S]["captures"].append(GraphRunner.captures - captures)
            stats[S]["images"] += S
            stats[S]["peak"] = max(stats[S]["peak"], torch.cuda.max_memory_allocated(device))
            last[S] = out
        # the pass breakdown from one more call with device events around every replay (not in the timed region)
        timer.wrap(pipe._runner)
        ops.start_census()
        call(S)
        stats[S]["passes"] = timer.collect()
        stats[S]["updates"] = {}
        for key, n in ops.stop_census().items():   # the eager latent-update launches of that call, per entry point
            if key[0].startswith(("latent_axpy", "latent_sgd_momentum")):
                stats[S]["updates"][key[0]] = stats[S]["updates"].get(key[0], 0) + n
    for S in sizes:
        st, out = stats[S], last[S]
        per_image = getattr(out, "unet_calls_per_image", [out.unet_calls])
        print(json.dumps({
            "metric": "prompts_per_pass" if mine.layouts else "seeds_per_pass", "seeds_per_pass": S, "layouts": mine.layouts,
            "use_optimizer": bool(mine.use_optimizer), "graph_captures_per_timed_call": st["captures"], "model": mine.model,
            "dtype": "float16", "graphs": True,
            "images_per_s": round(st["images"] / st["seconds"], 4), "ms_per_image": round(1e3 * st["seconds"] / st["images"], 2),
            "timed_images": st["images"], "pass_ms_at_batch": st["passes"],
            "update_launches_per_call": st["updates"], "unet_calls_per_image": per_image,
            "batched_passes": getattr(out, "batched_passes", None), "peak_memory_gib": round(st["peak"] / 2 ** 30, 3)}),
            flush=True)


def layout_state(k, rc, use_optimizer=False):
    """Layout k of the bench prompt as a GuidanceState: its boxes moved by k tenths of the image (kept inside it), shrink_factor
    and the threshold table varied, the rest of the bench's hyper-parameters unchanged."""
    import copy
    import re
    from guided_attention_amd import run
    from guided_attention_amd.pipeline_guided_attention import GuidanceState
    from guided_attention_amd.utils import shared_state as state

    def move(m):
        x, y, w, h = (float(v) for v in m.group(2).split(","))
        x, y = x + 0.1 * k, y + 0.05 * k
        x, y = (x if x + w <= 1.0 else x - (1.0 - w)), (y if y + h <= 1.0 else y - (1.0 - h))   # wrap inside the image
        return f"[{m.group(1)}:{x:.2f},{y:.2f},{w},{h}]"
    meta = re.sub(r"\[([^:\]]+):([^\]]+)\]", move, bench.META_PROMPT)
    saved = state.curHyperParams, state.config
    try:
        state.curHyperParams = dict(state.get_hyperparam_states()[0], meta_prompt=meta, shrink_factor=round(.15 - .05 * (k % 3), 2),
                                    thresholds={0: round(1.0 - 0.2 * (k % 3), 2), 10: 0.8})
        if use_optimizer:
            state.curHyperParams["use_optimizer"] = True
        cfg = copy.copy(rc)
        run.overrideConfig(cfg)
        run.parseMetaPrompt(cfg)
        return GuidanceState(cfg, state.curHyperParams)
    finally:
        state.curHyperParams, state.config = saved


if __name__ == "__main__":
    main()
