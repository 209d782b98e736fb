"""The VAE decode (GuidedAttention.decode_latents up to the clamp) on the framework path (vae.decode: MIOpen convolutions, NCHW
GroupNorm + SiLU, interpolate, scaled_dot_product_attention) against the own-kernel path (vae.decode_own, the
`own_vae_decode` switch), full SD decoder ch = (128, 256, 512, 512), f16, seeded random weights.

Cases: latents 64 x 64 with B = 1 and B = 4, 96 x 96 with B = 1.  Both paths run eager (the decode is not captured), warmed,
ALTERNATING in one process round by round, `iters` decodes between two device events; medians and spread over the rounds.
Launches per decode: the own path's from the census (ops.start_census), both paths' GPU kernels from torch.profiler in a run of
their own.  Parity: the small decoder of tests/test_vae_decode_gpu.py (ch = (64, 64, 128, 512), latents (2, 4, 16, 16)) on both
paths against the module's arithmetic in fp64 on the CPU, max abs / max |ref| before the clamp, f16 and bf16.

    python tools/micro/vae_decode_bench.py [--rounds 10] [--iters 3] [--out profiles/vae_decode.json]
"""
import argparse
import copy
import json
import statistics
import sys
from collections import Counter
from pathlib import Path

import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

CASES = [(1, 64, 64), (4, 64, 64), (1, 96, 96)]


def seeded(vae, seed):
    g = torch.Generator().manual_seed(seed)
    norm_params = {id(p) for m in vae.modules() if isinstance(m, nn.GroupNorm) for p in (m.weight, m.bias)}
    with torch.no_grad():
        for m in vae.modules():
            if isinstance(m, nn.GroupNorm):
                cg = m.num_channels // m.num_groups
                m.weight.copy_((0.6 + 0.8 * torch.rand(m.num_groups, generator=g)).repeat_interleave(cg))
                m.bias.copy_((0.3 * torch.randn(m.num_groups, generator=g)).repeat_interleave(cg))
        for n, p in vae.named_parameters():
            if n.endswith("bias") and id(p) not in norm_params:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return vae


def on_gpu(vae, dtype):
    from guided_attention_amd import fused_linear, ops
    from guided_attention_amd.vae import set_own_kernels
    vae.to("cuda", dtype)
    set_own_kernels(vae, ops, fused_linear)
    return vae


def parity(dtype):
    from guided_attention_amd.vae import AutoencoderKLDecoder
    vae = on_gpu(seeded(AutoencoderKLDecoder(ch=(64, 64, 128, 512)).init_weights_(), 7), dtype)
    lat = torch.randn((2, 4, 16, 16), generator=torch.Generator().manual_seed(41)).to("cuda", dtype)
    ref64 = copy.deepcopy(vae).cpu().double()
    with torch.no_grad():
        ref = ref64.decode(lat.double().cpu() / vae.scaling_factor)
        parent = vae.decode(lat / vae.scaling_factor)
    own = vae.decode_own(lat, 1.0 / vae.scaling_factor)
    err = lambda t: float((t.double().cpu() - ref).abs().max() / ref.abs().max())  # noqa: E731
    return {"err_own": err(own), "err_parent": err(parent)}


def gpu_kernels(fn):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and not e.name.lower().startswith(("memcpy", "memset", "copybuffer", "fillbuffer"))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "vae_decode.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_decode_bench needs the GPU: nothing is measured without one")
    from guided_attention_amd import ops
    from guided_attention_amd.vae import AutoencoderKLDecoder
    ops.load()
    ops.prepare_device("cuda")
    torch.backends.cudnn.benchmark = False     # as install_kernels leaves it
    result = {"what": "VAE decode up to the clamp, full SD decoder, f16, eager: framework path (vae.decode) against own kernels "
                      "(vae.decode_own), alternating rounds, device events",
              "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters_per_round": args.iters,
              "parity_small_decoder_max_abs_over_max_ref": {"f16": parity(torch.float16), "bf16": parity(torch.bfloat16)},
              "cases_BxHxW": {}}
    print(json.dumps(result["parity_small_decoder_max_abs_over_max_ref"]), flush=True)
    vae = on_gpu(seeded(AutoencoderKLDecoder().init_weights_(), 11), torch.float16)
    for B, h, w in CASES:
        lat = torch.randn((B, 4, h, w), generator=torch.Generator().manual_seed(h + B)).to("cuda", torch.float16)

        def framework():
            with torch.no_grad():
                return vae.decode(lat / vae.scaling_factor)

        def own():
            return vae.decode_own(lat, 1.0 / vae.scaling_factor)

        sides = {"framework": framework, "own": own}
        outs = {}
        for k, fn in sides.items():
            for _ in range(3):
                outs[k] = fn()
        torch.cuda.synchronize()
        agree = float((outs["own"].float() - outs["framework"].float()).abs().max() / outs["framework"].float().abs().max())
        del outs
        times = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, fn in sides.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    fn()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b) / args.iters / B)
        ops.start_census()
        own()
        census = Counter()
        for key, n in ops.stop_census().items():
            census[key[0]] += n
        entry = {"own_against_framework_max_rel_diff": agree}
        for k, fn in sides.items():
            entry[k] = {"ms_per_image_median": round(statistics.median(times[k]), 3), "ms_per_image_min": round(min(times[k]), 3),
                        "ms_per_image_max": round(max(times[k]), 3), "gpu_kernels_per_decode": gpu_kernels(fn)}
        entry["own"]["census_launches_per_decode"] = sum(census.values())
        entry["own"]["census"] = dict(census)
        entry["framework"]["census_launches_per_decode"] = 0
        entry["framework_over_own"] = round(entry["framework"]["ms_per_image_median"] / entry["own"]["ms_per_image_median"], 3)
        result["cases_BxHxW"][f"{B}x{h}x{w}"] = entry
        print(f"{B}x{h}x{w}", json.dumps(entry), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
