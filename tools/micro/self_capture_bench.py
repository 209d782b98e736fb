"""One self-attention layer under capture="reference", forward + backward with a cotangent on the output only (what every
guidance pass of the shipped loss does): the flash kernels that also write the probabilities (ops.SelfAttentionCaptureFusedQKV:
ga_self_attn_capture_fwd, ga_self_attn_bwd) against the materialising path (ptp_utils._materialised_attention: head-split
copies, bmm, multiply, softmax, bmm, merge copy, framework autograd back through all of it).

Shapes: the SD-1.x layers a reference store keeps, (B, H, N, D) = (1, 8, 1024, 80), (1, 8, 256, 160), (1, 8, 64, 160), fp16.
The attention alone: the projections in front of it are not part of either side.  Each side's forward + backward is captured
into one hipGraph; the sides are replayed interleaved, round by round, `iters` replays between two device events.  The GPU
kernels one forward + backward launches on each side are counted with torch.profiler in a run of their own.

    python tools/micro/self_capture_bench.py [--rounds 10] [--iters 100] [--out profiles/self_attn_capture.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

SHAPES = [(1, 8, 1024, 80), (1, 8, 256, 160), (1, 8, 64, 160)]


def sides_for(shape, dev):
    from guided_attention_amd import ops
    from guided_attention_amd.utils import ptp_utils
    B, H, N, D = shape
    C, scale = H * D, D ** -0.5
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(B, N, 3 * C, generator=g).to(dev, torch.float16).requires_grad_(True)
    q, k, v = (t.contiguous().detach().requires_grad_(True) for t in qkv.detach().split(C, dim=-1))
    w = torch.randn(B, N, C, generator=g).to(dev, torch.float16)

    def kernels():
        with torch.enable_grad():
            o, probs = ops.SelfAttentionCaptureFusedQKV.apply(qkv, H, scale)
            (d_qkv,) = torch.autograd.grad(o, [qkv], w)
        return o, probs, d_qkv

    def materialised():
        with torch.enable_grad():
            o, probs = ptp_utils._materialised_attention(q, k, v, H, scale)
            dq, dk, dv = torch.autograd.grad(o, [q, k, v], w)
        return o, probs, torch.cat([dq, dk, dv], dim=-1)

    return {"kernels": kernels, "materialised": materialised}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "self_attn_capture.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("self_capture_bench needs the GPU: nothing is measured without one")
    from guided_attention_amd import ops
    dev = torch.device("cuda", 0)
    ops.load()
    ops.prepare_device(dev)
    side = ops.side_stream(dev)
    ops.prepare_device(dev, side)
    try:
        clock_mhz = torch.cuda.clock_rate(dev)
    except Exception:   # the query needs a management library this installation may lack
        clock_mhz = None

    def summary(xs):
        return {"median_us": round(statistics.median(xs), 2), "min_us": round(min(xs), 2), "max_us": round(max(xs), 2)}

    shapes = {}
    for shape in SHAPES:
        sides = sides_for(shape, dev)
        # the two sides agree before anything is timed (fp16 roundings apart)
        ref = {k: fn() for k, fn in sides.items()}
        torch.cuda.synchronize()
        agree = {name: ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()
                 for name, a, b in zip(("o", "probs", "d_qkv"), ref["kernels"], ref["materialised"])}
        assert agree["o"] < 8e-3 and agree["probs"] < 4e-3 and agree["d_qkv"] < 2.4e-2, agree
        del ref
        graphs = {}
        for k, fn in sides.items():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with ops.no_gc(), torch.cuda.graph(graphs[k], stream=side):
                keep = fn()
            graphs[k].keep = keep   # the graph's outputs stay alive with it
        torch.cuda.synchronize()
        for gr in graphs.values():
            for _ in range(10):
                gr.replay()
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
        for k, fn in sides.items():   # a run of its own: tracing slows the host
            torch.cuda.synchronize()
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                     and not e.name.lower().startswith(("memcpy", "memset", "copybuffer", "fillbuffer"))]
            own = [n for n in names if "self_attn" in n]
            launches[k] = {"gpu_kernels": len(names), "own_kernels": len(own), "framework_kernels": len(names) - len(own)}
        med = {k: statistics.median(v) for k, v in replay.items()}
        shapes["x".join(map(str, shape))] = {
            "agreement_max_rel_diff": agree, "graph_replay_device_events": {k: summary(v) for k, v in replay.items()},
            "materialised_over_kernels": round(med["materialised"] / med["kernels"], 3), "launches": launches}
        del graphs
    result = {"what": "one captured self-attention layer, forward + backward with a cotangent on o only, fp16: "
                      "SelfAttentionCaptureFusedQKV against _materialised_attention + framework autograd",
              "device": torch.cuda.get_device_name(0), "shader_clock_mhz_at_start": clock_mhz, "rounds": args.rounds,
              "iters_per_round": args.iters, "shapes_BxHxNxD": shapes}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
