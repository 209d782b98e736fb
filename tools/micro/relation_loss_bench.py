"""One loss evaluation plus its backward, from the stored attention maps to the per-map gradient dP, for a prompt with box terms
and a `[CustomLoss:toLeftOf (a, b)]` relation (or another built-in one: --relation): GuidedAttention.fused_relation_loss off (aggregate launch + loss launch + the
plugin's torch graph, autograd back through all of it) against on (one relation launch each way).

Shape: 16 x 16 x 77, 5 stored maps of 8 heads, fp16 — what an SD-1.x guidance evaluation hands the loss.  Two timings per side,
both with the sides interleaved round by round (same process, same inputs):
  eager  host clock around `iters` evaluations ending in a device synchronise (what a run without hipGraphs pays)
  graph  the evaluation + backward captured into one hipGraph, `iters` replays between two device events (what the captured
         passes pay: no host in the loop)
and the GPU kernels one evaluation + backward launches on each side (torch.profiler, a run of its own).
--relation takes one name or several; with several, every relation's two sides share the rounds (all of them interleaved), and
the result's keys are NAME.off / NAME.on.

    python tools/micro/relation_loss_bench.py [--rounds 10] [--iters 200] [--out profiles/relation_loss.json]
    python tools/micro/relation_loss_bench.py --relation toLeftOf above --out profiles/relation_kinds.json
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

META_PROMPT = "a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55] near a cat and a dog [CustomLoss:{relation} (cat, dog)]"


def build(relation="toLeftOf"):
    from guided_attention_amd import ops, run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.text import WordTokenizer
    from guided_attention_amd.utils import shared_state as state
    dev = torch.device("cuda", 0)
    ops.load()
    ops.prepare_device(dev)
    pipe = GuidedAttention(SimpleNamespace(device=dev, dtype=torch.float16), None, None, None, WordTokenizer())
    cfg = RunConfig(meta_prompt=META_PROMPT.format(relation=relation), output_path="/tmp/ga_relation_bench")
    cfg.stable = pipe
    state.config = cfg
    state.curHyperParams = dict(state.hyperParameterOverrides)
    run.register_builtin_losses()
    run.parseMetaPrompt(cfg)
    pipe.bench_config = cfg
    g = torch.Generator().manual_seed(0)
    maps = [torch.softmax(torch.randn(8, 256, 77, generator=g) * 3, -1).to(dev, torch.float16).requires_grad_(True)
            for _ in range(5)]
    store = SimpleNamespace(get_average_attention=lambda: {"up_cross": maps[:3], "down_cross": maps[3:], "mid_cross": []})
    return pipe, store, maps


def evaluation(pipe, store, maps, on):
    """The device half of one evaluation and its backward to the stored maps -> (packed loss table, dP of the first map)."""
    from guided_attention_amd import ops
    from guided_attention_amd.utils import shared_state as state
    state.config = pipe.bench_config        # the prompt (and its relation) this pipeline was built for
    pipe.fused_relation_loss = on
    with torch.enable_grad():
        parts = pipe._aggregate_loss_device(store, 16, True, .5, 3, False)
        loss, custom = parts[1], parts[2]
        if not on:
            loss = loss + custom.to(loss.dtype).reshape(1)      # what _compute_loss forms on the plugin path
        grads = torch.autograd.grad(loss.sum(), maps)
    ops._image_broadcasts.clear()   # no capture backward consumes the per-image views here
    return parts[4], grads[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--relation", nargs="+", default=["toLeftOf"], choices=["toLeftOf", "toRightOf", "above", "below"])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "relation_loss.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("relation_loss_bench needs the GPU: nothing is measured without one")
    from guided_attention_amd import ops
    # one pipeline per relation, all on the same maps' values (the same seed); side -> (pipeline, store, maps, switch)
    prefix = (lambda name: "") if len(args.relation) == 1 else (lambda name: name + ".")
    sides, agree = {}, {}
    for name in args.relation:
        pipe, store, maps = build(name)
        sides[prefix(name) + "off"] = (pipe, store, maps, False)
        sides[prefix(name) + "on"] = (pipe, store, maps, True)
    # the two sides of a relation agree (the same loss, the same gradient) before anything is timed
    ref = {k: evaluation(*side) for k, side in sides.items()}
    torch.cuda.synchronize()
    for name in args.relation:
        off, on = ref[prefix(name) + "off"], ref[prefix(name) + "on"]
        total_off, total_on = off[0].float().cpu()[-2:].sum().item(), on[0].float().cpu()[-2:].sum().item()
        g_off, g_on = off[1].float(), on[1].float()
        agree[name] = {"loss_off": total_off, "loss_on": total_on, "relation_loss_on": on[0].float().cpu()[-1].item(),
                       "grad_max_rel_diff": ((g_on - g_off).abs().max() / g_off.abs().max()).item()}
        assert abs(total_on - total_off) <= 1e-4 * abs(total_off) and agree[name]["grad_max_rel_diff"] < 2e-2, agree   # fp16 dP
    if len(args.relation) == 1:
        agree = agree[args.relation[0]]
    maps = next(iter(sides.values()))[2]

    for _ in range(20):   # warm-up of every shape the sides launch
        for side in sides.values():
            evaluation(*side)
    torch.cuda.synchronize()
    eager = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, side in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                evaluation(*side)
            torch.cuda.synchronize()
            eager[k].append((time.perf_counter() - t0) / args.iters * 1e6)

    graphs, side = {}, ops.side_stream(maps[0].device)
    ops.prepare_device(maps[0].device, side)
    for k, what in sides.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                evaluation(*what)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[k] = torch.cuda.CUDAGraph()
        with ops.no_gc(), torch.cuda.graph(graphs[k], stream=side):
            keep = evaluation(*what)   # noqa: F841  the graph's outputs stay alive with it
        graphs[k].keep = keep
    torch.cuda.synchronize()
    for g in graphs.values():
        for _ in range(20):
            g.replay()
    torch.cuda.synchronize()
    replay = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k in sides:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                graphs[k].replay()
            b.record()
            b.synchronize()
            replay[k].append(a.elapsed_time(b) / args.iters * 1e3)

    launches = {}
    for k, what in sides.items():   # a run of its own: tracing slows the host
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            evaluation(*what)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                 and not e.name.lower().startswith(("memcpy", "memset", "copybuffer", "fillbuffer"))]
        own = [n for n in names if "smooth_loss" in n or "aggregate_" in n]
        launches[k] = {"gpu_kernels": len(names), "own_loss_kernels": len(own), "framework_kernels": len(names) - len(own)}

    def summary(xs):
        return {"median_us": round(statistics.median(xs), 2), "min_us": round(min(xs), 2), "max_us": round(max(xs), 2)}
    result = {"what": "one loss evaluation + backward, stored maps -> dP, 16x16x77, 5 maps x 8 heads, fp16; "
                      + " / ".join(args.relation) + " + 3 box tokens",
              "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters_per_round": args.iters,
              "agreement": agree,
              "eager_host_clock": {k: summary(v) for k, v in eager.items()},
              "graph_replay_device_events": {k: summary(v) for k, v in replay.items()},
              "launches_per_evaluation": launches}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
