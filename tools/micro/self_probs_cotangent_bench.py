"""One self-attention layer under capture="reference", forward + backward with a cotangent on the output AND a head-broadcast
cotangent on the stored probabilities (what a loss on aggregate_attention(..., is_cross=False) sends back): the flash backward
that takes the cotangent itself (ops.SelfAttentionCaptureFusedQKV: ga_self_attn_capture_fwd, ga_self_attn_bwd_dp) against the
arithmetic this branch ran before — the plain flash backward, then per (batch, head) the f32 terms dS = P o (dP - rowsum(P o dP)),
dq += scale dS K, dk += scale dS^T Q on framework kernels (two mm per head) and two slice adds.  That arithmetic is restated
here, privately, from the stored P: the package no longer has it.

Shapes, protocol and output format are tools/micro/self_capture_bench.py's: (B, H, N, D) = (1, 8, 1024, 80), (1, 8, 256, 160),
(1, 8, 64, 160), fp16; each side's forward + backward is one hipGraph; the sides are replayed interleaved, round by round,
`iters` replays between two device events.

    python tools/micro/self_probs_cotangent_bench.py [--rounds 10] [--iters 100] [--out profiles/self_attn_probs_cotangent.json]
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


def framework_terms(q, k, probs, d_probs, heads, scale):
    """What the cotangent on the probabilities adds to dq and dk, per (batch, head) in f32 from the stored P.
    q, k: (B, N, heads, d) views -> two f32 (B, N, heads, d) tensors."""
    B, N, H, d = q.shape
    eq = torch.empty((B, N, H, d), dtype=torch.float32, device=q.device)
    ek = torch.empty_like(eq)
    for b in range(B):
        for h in range(H):
            p = probs[b * H + h].float()
            ds = p * d_probs[b * H + h].float()
            ds -= p * ds.sum(dim=-1, keepdim=True)
            eq[b, :, h] = torch.mm(ds, k[b, :, h].float()) * scale
            ek[b, :, h] = torch.mm(ds.t(), q[b, :, h].float()) * scale
    return eq, ek


def sides_for(shape, dev):
    from guided_attention_amd import ops
    B, H, N, D = shape
    C, scale = H * D, D ** -0.5
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(B, N, 3 * C, generator=g).to(dev, torch.float16).requires_grad_(True)
    w = torch.randn(B, N, C, generator=g).to(dev, torch.float16)
    d_p = torch.randn(N, N, generator=g).to(dev, torch.float16).unsqueeze(0).expand(B * H, N, N)   # one map, stride 0 over heads

    def kernels():
        with torch.enable_grad():
            o, probs = ops.SelfAttentionCaptureFusedQKV.apply(qkv, H, scale)
            (d_qkv,) = torch.autograd.grad([o, probs], [qkv], [w, d_p])
        return o, probs, d_qkv

    def framework():
        with torch.enable_grad():
            o, probs = ops.SelfAttentionCaptureFusedQKV.apply(qkv, H, scale)
            (d_qkv,) = torch.autograd.grad(o, [qkv], w)                       # the plain flash backward
        with torch.no_grad():
            split = lambda lo: qkv[..., lo:lo + C].view(B, N, H, D)  # noqa: E731
            eq, ek = framework_terms(split(0), split(C), probs, d_p, H, scale)
            d_qkv[..., :C] = eq.view(B, N, C).add_(d_qkv[..., :C])
            d_qkv[..., C:2 * C] = ek.view(B, N, C).add_(d_qkv[..., C:2 * C])
        return o, probs, d_qkv

    return {"kernels": kernels, "framework": framework}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "self_attn_probs_cotangent.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("self_probs_cotangent_bench needs the GPU: nothing is measured without one")
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
                 for name, a, b in zip(("o", "probs", "d_qkv"), ref["kernels"], ref["framework"])}
        assert agree["o"] == 0 and agree["probs"] == 0 and agree["d_qkv"] < 2.4e-2, agree
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
            "framework_over_kernels": round(med["framework"] / med["kernels"], 3),
            "kernels_within_3_percent_of_framework": med["kernels"] <= 1.03 * med["framework"], "launches": launches}
        del graphs
    result = {"what": "one captured self-attention layer, forward + backward with a cotangent on o and a head-broadcast cotangent "
                      "on the probabilities, fp16: ga_self_attn_bwd_dp against the flash backward + per-head framework terms",
              "device": torch.cuda.get_device_name(0), "shader_clock_mhz_at_start": clock_mhz, "rounds": args.rounds,
              "iters_per_round": args.iters, "shapes_BxHxNxD": shapes}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
