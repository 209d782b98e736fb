#!/usr/bin/env python3
"""bench.py — guided images/sec of the guided-attention hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes the last timed step's outputs if --dump-outputs is given and
prints the result line.  --full also measures what the headline does not need: the two-pass figure, the per-kernel
roofline micro-replays and the CPU baseline (--two-pass-steps 0, --no-roofline and --no-cpu-baseline still drop each).

N > 1: either launched by `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` (RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* in the environment), or run directly — then this process touches no GPU and starts the N ranks
itself as child processes (one per GPU, rendezvous on 127.0.0.1), relays rank 0's JSON line and exits with the worst
return code.

One "step" = one guided image: the full 50-step DDIM guided sampling of the SD-1.x UNet at 512^2
(latent 64^2), prompt 'a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]', guidance 7.5, the
reference's shipped hyper-parameters (thresholds {0:1.0}, recurse_steps 3, max 10 refinement
iterations), fp16, timed from after prompt encoding to the final latents (the VAE
decode is outside the metric).  Synthetic inputs: seeded random-init UNet weights (no checkpoint
offline), synthetic prompt embeddings, host-generated initial latents and re-noise tensors.
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

META_PROMPT = "a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]"
META_PROMPT_SD21 = "a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55] under a [moon:.35,.05,.35,.35]"
META_PROMPT_SDXL = "a [robot:.6,.3,.4,.55] and a blue [vase:.2,.3,.4,.55]"   # BASELINE config 5: 2 guided tokens
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2, help="timed guided images per GPU")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="default", choices=["default", "every-step"])
    ap.add_argument("--model", default=os.environ.get("GA_BENCH_MODEL", "sd15"), choices=["sd15", "sd21", "sdxl", "tiny"],
                    help="sd21 = BASELINE config 4: SD-2.1 UNet shapes at 768^2 (latent 96^2, maps 24x24), 3 box tokens; "
                         "sdxl = config 5: SDXL-base UNet shapes at 1024^2 (latent 128^2, maps 32x32), 2 tokens, bf16")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--guidance-forward", default="full", choices=["full", "truncated"])
    ap.add_argument("--skip-unused-guidance", action="store_true")
    ap.add_argument("--eager", action="store_true", help="launch every kernel from the host instead of replaying hipGraphs")
    ap.add_argument("--no-joint-pass", action="store_true",
                    help="run the loss-only guidance forward and the CFG pair as two passes (B=1, B=2) instead of one B=3 pass")
    ap.add_argument("--miopen-search", action="store_true",
                    help="A/B only: MIOpen's exhaustive solver search (cudnn.benchmark) for the few convolutions left on the library")
    ap.add_argument("--no-run-ahead", action="store_true",
                    help="refinement loop reads each loss table back before it enqueues the backward / update / next evaluation")
    ap.add_argument("--two-pass-steps", type=int, default=1,
                    help="--full: after the timed region, also time this many images with the two-pass form of the loss-only "
                         "steps and report it beside the headline (0 = skip)")
    ap.add_argument("--no-roofline", action="store_true",
                    help="--full without the per-shape micro-replays behind `roofline` (profiling runs: nothing but images in the trace)")
    ap.add_argument("--launch-timeout", type=float, default=3300.0,
                    help="self-launched ranks (--gpus N run directly) are terminated after this many seconds")
    ap.add_argument("--launch-check", action="store_true",
                    help="only exercise the N-rank launch + rendezvous (gloo when no GPU is visible) and print one line")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also run the two-pass leg, the roofline micro-replays and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (rank 0) as DIR/<name>.npy: latents (float32), "
                         "unet_calls (float64, in the order of PipelineOutput.unet_calls)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


# ------------------------------------------------------------------------------------------------ N-rank self-launch
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def rank_envs(n, port, base=None):
    """Environment of each of the n ranks of one node (what torch.distributed.run would set)."""
    base = dict(os.environ if base is None else base)
    envs = []
    for r in range(n):
        e = dict(base)
        e.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                 MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GA_BENCH_SELF_LAUNCHED="1")
        e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL needs on this driver
        e.setdefault("OMP_NUM_THREADS", str(max(1, usable_cores() // n)))
        envs.append(e)
    return envs


def launch_ranks(n, argv, deadline_s=3300.0):
    """Start n copies of this script, one per GPU.  The parent has made no GPU call and execs nothing: children are
    ordinary subprocesses; rank 0 inherits stdout (its JSON line is THE line), the other ranks' stdout is dropped,
    stderr is shared.  Returns the worst child return code; if one rank dies the others are terminated, and so are all
    of them when the deadline passes or the parent is interrupted (no rank is left holding a GPU or the port)."""
    port = free_port()
    procs = []
    worst = 0
    try:
        for r, env in enumerate(rank_envs(n, port)):
            procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve()), *argv], env=env,
                                          stdout=None if r == 0 else subprocess.DEVNULL))
        alive = set(range(n))
        t_end = time.monotonic() + deadline_s
        while alive:
            for r in sorted(alive):
                rc = procs[r].poll()
                if rc is None:
                    continue
                alive.discard(r)
                if rc != 0:
                    worst = worst or rc
                    for o in alive:          # a rank failed: the others would wait in a collective forever
                        procs[o].terminate()
            if alive and time.monotonic() > t_end:
                print(f"bench.py: ranks {sorted(alive)} still running after {deadline_s:.0f} s: terminating", file=sys.stderr)
                worst = worst or 124
                break
            time.sleep(0.2)
    finally:
        stragglers = [p for p in procs if p.poll() is None]
        for p in stragglers:
            p.terminate()
        for p in stragglers:
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                p.kill()
    return worst


def launch_check():
    """The launch path without the workload: rendezvous, one all-reduce, one line (CPU: gloo)."""
    from guided_attention_amd import parallel
    import torch.distributed as dist
    rank, world, local = parallel.init_distributed()
    dev = torch.device("cuda", local) if torch.cuda.is_available() else torch.device("cpu")
    x = torch.tensor([float(rank + 1)], device=dev)
    if world > 1:
        dist.all_reduce(x)
        dist.barrier()
    if rank == 0:
        print(json.dumps({"launch_check": True, "world": world, "backend": dist.get_backend() if world > 1 else None,
                          "sum": float(x), "self_launched": os.environ.get("GA_BENCH_SELF_LAUNCHED") == "1"}))
    if world > 1:
        dist.destroy_process_group()


def build_pipeline(args, device, rank, world):
    from guided_attention_amd import parallel
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.text import SyntheticTextEncoder, WordTokenizer
    from guided_attention_amd.unet import UNet2DConditionModel, UNetConfig
    import torch.distributed as dist
    cfg = {"sd15": UNetConfig.sd15, "sd21": UNetConfig.sd21, "sdxl": UNetConfig.sdxl}.get(
        args.model, lambda: UNetConfig.tiny(64, 768))()
    dtype = torch.bfloat16 if args.model == "sdxl" else torch.float16   # BASELINE config 5 is quoted in bf16
    with torch.device(device):
        unet = UNet2DConditionModel(cfg)
    unet = unet.to(dtype)
    if rank == 0:
        unet.init_weights_(seed=0)       # seeded random weights of the architecture; the other ranks receive them
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    n_msgs = parallel.broadcast_module_(unet)  # RCCL over xGMI: the only start-up collective
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    bcast_s = time.perf_counter() - t0
    nbytes = sum(p.numel() * p.element_size() for p in unet.parameters())
    pipe = GuidedAttention(unet, None, None, SyntheticTextEncoder(cfg.cross_attention_dim), WordTokenizer())
    pipe.to(device, dtype)
    if cfg.addition_embed_type == "text_time":   # SDXL: synthetic pooled text embeddings + the 1024^2 size/crop ids
        g = torch.Generator("cpu").manual_seed(4321)
        pooled = torch.randn(2, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim, generator=g)
        side = float(cfg.sample_size * 8)
        unet.set_added_cond(pooled, torch.tensor([[side, side, 0.0, 0.0, side, side]] * 2))
    pipe.guidance_forward = args.guidance_forward
    pipe.skip_unused_guidance = args.skip_unused_guidance
    pipe.use_graphs = not args.eager
    pipe.batch_loss_only_guidance = not args.no_joint_pass
    pipe.speculative_refinement = not args.no_run_ahead
    if args.miopen_search:
        torch.backends.cudnn.benchmark = True
    return pipe, cfg, {"messages": n_msgs, "seconds": round(bcast_s, 4), "bytes": nbytes,
                       "timed": "between two barriers" if world > 1 else "single rank: no collective"}


def make_run(args, pipe, cfg, device):
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.utils import helpers, ptp_utils, shared_state as state
    rc = RunConfig(meta_prompt={"sd21": META_PROMPT_SD21, "sdxl": META_PROMPT_SDXL}.get(args.model, META_PROMPT),
                   output_path="/tmp/ga_bench_out", half_precision=True, n_inference_steps=args.ddim_steps)
    if args.model in ("sd21", "sdxl"):
        # the (latent/4)^2 maps: 24x24 of the 96^2 latent, 32x32 of the 128^2 latent (synthetic embeddings: no EOT slice)
        rc.attention_res = cfg.sample_size // 4
    if args.workload == "every-step":
        rc.only_update_on_threshold_steps = False
        rc.max_iter_to_alter = 25
    rc.stable = pipe
    state.curHyperParams = state.get_hyperparam_states()[0]
    run.overrideConfig(rc)        # thresholds := {0: 1.0}, as the reference does at run time
    run.parseMetaPrompt(rc)
    g = torch.Generator("cpu").manual_seed(1234)
    embeds = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).to(device, pipe.unet.dtype)
    lat_side = cfg.sample_size

    def prepare(seed):
        """The inputs of one image, host-generated (shared with the CPU oracle: SURVEY section 8d) and made resident in HBM
        BEFORE the timed region: initial latents and the re-noise tensors of the recurse rounds."""
        gs = torch.Generator("cpu").manual_seed(seed)
        latents = torch.randn(1, 4, lat_side, lat_side, generator=gs).to(device, pipe.unet.dtype)
        noise = [torch.randn(1, 4, lat_side, lat_side, generator=gs).to(device, pipe.unet.dtype)
                 for _ in range(2 * args.ddim_steps)]
        return seed, latents, noise

    def one_image(prepared):
        seed, latents, noise = prepared
        noise = list(noise)       # the pipeline consumes the list
        helpers.log_clear()
        state.cur_seed = seed
        controller = ptp_utils.AttentionStore()
        ptp_utils.register_attention_control(pipe, controller)
        return pipe(prompt=None, prompt_embeds=embeds[1:2], negative_prompt_embeds=embeds[0:1],
                    attention_store=controller, attention_res=rc.attention_res, guidance_scale=rc.guidance_scale,
                    num_inference_steps=rc.n_inference_steps, max_iter_to_alter=rc.max_iter_to_alter,
                    thresholds=rc.thresholds, scale_factor=rc.scale_factor, scale_range=rc.scale_range,
                    smooth_attentions=rc.smooth_attentions, sigma=rc.sigma, kernel_size=rc.kernel_size,
                    latents=latents, renoise_noise=noise, output_type="latent")

    one_image.prepare = prepare
    return one_image, rc, embeds


def usable_cores():
    """Host cores this process may actually use: the affinity mask capped by the cgroup CPU quota
    (os.cpu_count() reports the whole host and oversubscribes a container)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = Path("/sys/fs/cgroup/cpu.max").read_text().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: ~2.5 PF dense fp16/bf16


def kernel_work(key):
    """Algorithmic work of ONE call of a hand-written kernel: ("hbm", bytes) or ("mfma", flops).
    capture fwd  = Q + O + K + V (+ P when stored);  capture bwd = Q + dO + dQ + K + V (+ the broadcast dP map)
    self-attn    = 4 N^2 D flops per head forward, 2.5x that for the backward (5 matrix products, recompute not counted)
    GroupNorm    = read x + write y (fwd), read x, dy + write dx (bwd)."""
    kind, B, H, N, Kt, D, flag, dt = key
    esz = 4 if dt == "torch.float32" else 2
    if kind in ("geglu_fwd", "geglu_bwd"):            # B = rows, D = F: x [rows][2F] in, y [rows][F] out (bwd: + dy, dx)
        return "hbm", esz * B * D * (3 if kind == "geglu_fwd" else 5)
    if kind == "bias_residual_add":                  # y + residual in, out
        return "hbm", esz * B * D * 3
    if kind == "add_layer_norm_fwd":                 # (a,) x in; (x_new,) y out
        return "hbm", esz * B * D * (4 if flag else 2)
    if kind == "add_layer_norm_bwd":                 # row, dy (, g_res) in; dx out
        return "hbm", esz * B * D * (4 if flag else 3)
    if kind == "conv3x3":                            # B, H = Cin, N = H*W, Kt = stride, D = Cout: 2 * M * 9 Cin * Cout
        return "mfma", 2.0 * B * (N // (Kt * Kt)) * 9 * H * D
    if kind in ("conv3x3_thin_in", "conv3x3_thin_out"):   # conv_in / conv_out: H = Cin, N = H*W, D = Cout: x in, y out
        return "hbm", esz * B * N * (H + D)
    if kind == "linear":                             # B = M, H = K, D = N (rows of W): 2 M K N whatever is folded in
        return "mfma", 2.0 * B * H * D
    if kind in ("aggregate_maps", "aggregate_loss_fwd"):   # H = head-maps in all, N = pixels, Kt = context tokens: maps in, A out
        return "hbm", esz * H * N * Kt + 4 * N * Kt
    if kind == "smooth_loss_fwd":                    # A (f32) in, < 1 KB out   (78.8 KB at 16 x 16 x 77)
        return "hbm", 4 * N * Kt
    if kind == "smooth_loss_bwd":                    # A in, dA out (+ the dtype-cast broadcast map)
        return "hbm", 8 * N * Kt + (esz * N * Kt if flag else 0)
    if kind in ("latent_axpy", "latent_axpby"):      # latents, grad in; latents out  (98 KB at 16 384 fp16 elements)
        return "hbm", 3 * esz * N
    if kind == "cfg_ddim_step":                      # eps_uncond, eps_text, x in; x_prev (, x0) out
        return "hbm", (5 if flag else 4) * esz * N
    if kind.startswith("group_norm"):
        elems = B * N * D  # here H = groups, N = pixels, D = channels
        return "hbm", esz * elems * (3 if kind == "group_norm_bwd" else 2)   # _fwd and _apply (statistics from the producer): x in, y out
    C = H * D
    if kind == "attn_capture_fwd":
        return "hbm", esz * (2 * B * N * C + 2 * B * Kt * C + (B * H * N * Kt if flag else 0))
    if kind == "attn_capture_bwd":
        return "hbm", esz * (3 * B * N * C + 2 * B * Kt * C + (N * Kt if flag else 0))
    flops = 4.0 * B * H * N * N * D
    return "mfma", flops * (1.0 if kind == "self_attn_fwd" else 2.5)


def pmc_traffic(kernel, model, shape):
    """HBM bytes per launch of the dominant kernel from the committed PMC run of THIS model's dominant shape
    (profiles/r2_pmc_traffic_<model>.json: FETCH_SIZE and WRITE_SIZE collected in separate rocprofv3 --pmc passes with
    the gfx950 corrections of MI355X_MICROARCH.md applied by tools/pmc_summary.py).  None when no PMC profile of that
    kernel AND shape is committed — the field is never filled from another model's or another shape's run."""
    for rnd in ("r4", "r3", "r2"):      # this round's PMC run; earlier rounds' for kernels that have not changed since
        try:
            doc = json.loads((ROOT / "profiles" / f"{rnd}_pmc_traffic_{model}.json").read_text())
            for k in doc["kernels"]:
                if k["kernel"] == kernel and all(k["shape"].get(x) == shape.get(x) for x in ("B", "H", "N", "D")):
                    return {"hbm_bytes": k["hbm_bytes_corrected"], "algorithmic_bytes": k["algorithmic_bytes"],
                            "shape": k["shape"], "source": f"profiles/{rnd}_pmc_traffic_{model}.json"}
        except (OSError, KeyError, ValueError):
            pass
    return None


def roofline_entry(census, ops, model="sd15"):
    """Dominant hand-written kernel = the ga_* entry point with the largest total time over the timed region.
    achieved = sum of algorithmic work over its calls / sum of their durations; each shape's duration is measured by a
    back-to-back hipGraph replay between two HIP events on the launch stream; the convolution replays rotate over enough
    weight copies to exceed the Infinity Cache, because in the pipeline its weights are cold (the weighted mean equals what
    `rocprofv3 --kernel-trace --stats` reports as the kernel's AverageNs: profiles/)."""
    per_kind = {}
    for key, count in census.items():
        us = ops.replay_launch_us(key)
        bound, work = kernel_work(key)
        d = per_kind.setdefault(key[0], {"bound": bound, "time_us": 0.0, "work": 0.0, "calls": 0, "shapes": []})
        d["time_us"] += us * count
        d["work"] += work * count
        d["calls"] += count
        rate = work / us / 1e3 if bound == "hbm" else work / us / 1e6  # GB/s or TFLOP/s
        d["shapes"].append({"B": key[1], "H": key[2], "N": key[3], "D": key[5], "flag": key[6], "calls": count,
                            "call_us": round(us, 2), "rate": round(rate, 1)})
    if not per_kind:
        return None

    def summary(kind, d):
        if d["bound"] == "hbm":
            achieved, peak, unit = d["work"] / d["time_us"] / 1e3, HBM_PEAK_GBS, "GB/s"
        else:
            achieved, peak, unit = d["work"] / d["time_us"] / 1e6, MFMA_PEAK_TFLOPS, "TFLOP/s"
        return {"bound": d["bound"], "kernel": "ga_" + kind, "achieved": round(achieved, 1), "peak": peak, "unit": unit,
                "frac": round(achieved / peak, 4), "avg_call_us": round(d["time_us"] / d["calls"], 2),
                "calls": d["calls"], "total_ms": round(d["time_us"] / 1e3, 2)}

    kind, d = max(per_kind.items(), key=lambda kv: kv[1]["time_us"])
    out = summary(kind, d)
    out["shapes"] = sorted(d["shapes"], key=lambda x: -x["calls"] * x["call_us"])[:6]
    out["traffic"] = pmc_traffic("ga_" + kind, model, out["shapes"][0])
    out["other_kernels"] = [summary(k, v) for k, v in sorted(per_kind.items(), key=lambda kv: -kv[1]["time_us"]) if k != kind]
    return out


def cpu_model_name():
    try:
        for line in Path("/proc/cpuinfo").read_text().splitlines():
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _timed(fn, reps):
    """One untimed warm-up call, then `reps` timed calls -> (median seconds, [seconds])."""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2], ts


def cpu_baseline(args, cfg, calls, rc, reps=3):
    """The oracle (CPU fp32 restatement, oracle/pipeline.py) on the host cores: per pass kind one warm-up and `reps`
    timed repetitions of a guidance evaluation (forward with autograd + loss), a backward to the latents and a CFG
    forward of the SAME UNet shape (medians), extrapolated with the GPU run's per-image call counts; the
    reference-style Python-pixel-loop loss (oracle.loss.loss_reference_loops) is timed as its own field, because the
    vectorised oracle loss is far faster than what the reference executes."""
    from oracle import loss as oloss
    from oracle.pipeline import GuidedSampler
    from guided_attention_amd.unet import UNet2DConditionModel
    cores = usable_cores()
    torch.set_num_threads(cores)
    unet = UNet2DConditionModel(cfg).init_weights_(seed=0).float()
    for p in unet.parameters():
        p.requires_grad_(False)
    if cfg.addition_embed_type == "text_time":
        g0 = torch.Generator("cpu").manual_seed(4321)
        pooled = torch.randn(2, cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim, generator=g0)
        side = float(cfg.sample_size * 8)
        unet.set_added_cond(pooled, torch.tensor([[side, side, 0.0, 0.0, side, side]] * 2))
        reps = 1   # a 2.6 B-parameter fp32 forward takes the better part of a minute on the host: one repetition
    from guided_attention_amd.utils import helpers
    entries = []      # the guided tokens of the GPU run's own meta-prompt (rc.token_dict), as plain data
    for idx, info in rc.token_dict.items():
        box = info["loss_type"] == helpers.AnnotationType.BOX
        entries.append({"index": idx, "kind": "BOX" if box else "COOR",
                        "geom": info["loss"].as_tuple() if box else tuple(info["loss"]), "subprompt": info["subprompt"]})
    plan = oloss.TokenPlan(entries)
    s = GuidedSampler(unet, plan, thresholds={0: 1.0}, steps=args.ddim_steps, attention_res=rc.attention_res)
    g = torch.Generator("cpu").manual_seed(1234)
    embeds = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    lat = torch.randn(1, 4, cfg.sample_size, cfg.sample_size, generator=torch.Generator("cpu").manual_seed(0))
    box = {}

    def fwd():
        with torch.enable_grad():
            box["lat"], box["r"], _ = s._evaluate(lat, 981, embeds[1:2])

    def bwd():
        with torch.enable_grad():
            s._update(box["lat"], box["r"]["loss"], 20.0)

    def cfg_fwd():
        with torch.no_grad():
            unet(torch.cat([lat] * 2), 981, encoder_hidden_states=embeds)

    per, raw = {}, {}
    per["fwd_b1_grad"], raw["fwd_b1_grad"] = _timed(fwd, reps)
    per["bwd"], raw["bwd"] = _timed(bwd, reps)
    per["fwd_b2"], raw["fwd_b2"] = _timed(cfg_fwd, reps)
    sec_per_image = sum(per[k] * calls[k] for k in per)
    # the loss the way the reference evaluates it (Python loops over the res x res pixels, scalar tensor ops)
    A = torch.softmax(torch.randn(rc.attention_res, rc.attention_res, 77, generator=g), -1)

    def loop_loss():
        a = A.clone().requires_grad_(True)
        r = oloss.loss_reference_loops(a * 1.0, plan)
        box["loop_r"], box["loop_a"] = r, a

    def loop_loss_bwd():
        torch.autograd.grad(box["loop_r"]["loss"], [box["loop_a"]], retain_graph=True)

    def vec_loss():
        oloss.loss_torch(A, plan)

    loop_s, _ = _timed(loop_loss, reps)
    loop_bwd_s, _ = _timed(loop_loss_bwd, reps)
    vec_s, _ = _timed(vec_loss, reps)
    evals = calls.get("loss_evals", calls["fwd_b1_grad"])
    with_loops = sec_per_image + evals * (loop_s - vec_s) + calls["bwd"] * loop_bwd_s
    return {"value": 1.0 / sec_per_image, "unit": "images/s", "cores": cores, "cpu_model": cpu_model_name(),
            "threads": torch.get_num_threads(), "kind": "port",
            "sample": f"per pass kind 1 warm-up + {reps} timed repetitions (median) of: guidance forward+loss (autograd), "
                      f"backward to latents, CFG forward (B=2) of the same {args.model} UNet in fp32 on the host, "
                      f"extrapolated with the GPU run's per-image call counts { {k: calls[k] for k in per} }",
            "seconds_per_kind": {k: round(v, 3) for k, v in per.items()},
            "seconds_per_kind_all": {k: [round(x, 3) for x in v] for k, v in raw.items()},
            "seconds_per_image": round(sec_per_image, 1),
            "reference_style_loop_loss": {"fwd_ms": round(loop_s * 1e3, 2), "bwd_ms": round(loop_bwd_s * 1e3, 2),
                                          "vectorised_oracle_fwd_ms": round(vec_s * 1e3, 2),
                                          "images_per_s_with_loop_loss": 1.0 / with_loops}}


def dump_outputs(out_dir, latents, calls):
    """What a caller of the timed path receives from its last step, as .npy files (64 KB at SD-1.x, 256 KB at SDXL)."""
    import numpy as np
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    np.save(out_dir / "latents.npy", latents.detach().float().cpu().numpy())
    np.save(out_dir / "unet_calls.npy", np.array([calls[k] for k in calls], dtype=np.float64))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse(argv)
    if args.gpus > 1 and "RANK" not in os.environ:
        # run directly with --gpus N: start the N ranks ourselves.  Nothing above touched the GPU.
        raise SystemExit(launch_ranks(args.gpus, argv, args.launch_timeout))
    if args.launch_check:
        return launch_check()
    from guided_attention_amd import ops, parallel
    rank, world, local = parallel.init_distributed()
    if world > 1:
        # one MIOpen user database / kernel cache per rank: N processes benchmarking the same conv shapes at the same
        # time otherwise queue on the file locks of one shared database
        os.environ.setdefault("MIOPEN_USER_DB_PATH", f"/tmp/ga_miopen_{os.getuid()}_{local}")
        os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", f"/tmp/ga_miopen_{os.getuid()}_{local}/cache")
        os.makedirs(os.environ["MIOPEN_CUSTOM_CACHE_DIR"], exist_ok=True)
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the guided-attention path has no CPU fallback")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    ops.load()
    pipe, cfg, bcast = build_pipeline(args, device, rank, world)
    one_image, rc, _ = make_run(args, pipe, cfg, device)
    import torch.distributed as dist

    seed_of = lambda j: rank + world * j   # seeds striped by rank (weak scaling: K images per GPU)
    first_image_s = None
    for j in range(args.warmup):
        prepared = one_image.prepare(1000 + seed_of(j))
        torch.cuda.synchronize()
        tw = time.perf_counter()
        one_image(prepared)
        torch.cuda.synchronize()
        if j == 0:   # cold: hipGraph capture, library algorithm search, weight packs, text K/V and timestep caches all inside
            first_image_s = time.perf_counter() - tw
    inputs = [one_image.prepare(seed_of(j)) for j in range(args.steps)]   # resident in HBM before the timed region
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    if args.full:
        ops.start_census()   # the roofline's launch census
    t0 = time.perf_counter()
    calls = None
    finals = []
    for j in range(args.steps):
        out = one_image(inputs[j])
        finals.append(out.latents)
        calls = out.unet_calls
    torch.cuda.synchronize()
    t_mine = time.perf_counter() - t0
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    census = ops.stop_census()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, finals[-1], calls)
    per_rank = [args.steps / t_mine]
    if world > 1:
        tmax = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax)
        mine = torch.tensor([args.steps / t_mine], device=device, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [float(x) for x in allr]
    gathered = parallel.gather_tensors(finals)  # the end-of-run gather of the final latents (32 KB each)
    ok = all(torch.isfinite(f).all().item() for f in finals)
    if world > 1:
        okt = torch.tensor([1.0 if ok else 0.0], device=device)
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        ok = bool(okt.item() > 0)
    two_pass = None
    if args.full and world == 1 and args.two_pass_steps > 0 and pipe.batch_loss_only_guidance and pipe.use_graphs:
        # the strict two-pass form of the loss-only steps (B=1 guidance forward, then the B=2 CFG pass), quoted
        # beside the headline; outside the timed region (its graphs are captured in an untimed image first)
        pipe.batch_loss_only_guidance = False
        one_image(one_image.prepare(2000))
        inputs2 = [one_image.prepare(3000 + j) for j in range(args.two_pass_steps)]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for j in range(args.two_pass_steps):
            one_image(inputs2[j])
        torch.cuda.synchronize()
        two_pass = args.two_pass_steps / (time.perf_counter() - t1)
        pipe.batch_loss_only_guidance = True
    if rank == 0:
        n_images = args.steps * world
        roof = roofline_entry(census, ops, args.model) if args.full and not args.no_roofline else None
        flops_per_fwd = {"sd15": 0.803e12, "sd21": 2.149e12}.get(args.model)
        names = {"sd21": ("guided images/sec (50-step SD-2.1 768^2)", "SD-2.1 UNet 768^2 (latent 96^2)"),
                 "sdxl": ("guided images/sec (50-step SDXL-base 1024^2)", "SDXL-base UNet 1024^2 (latent 128^2)"),
                 "tiny": ("guided images/sec (50-step reduced-width UNet 512^2)", "1/10-width SD-1.x UNet 512^2")}
        metric, shape = names.get(args.model, ("guided images/sec (50-step SD-1.5 512^2)", "SD-1.x UNet 512^2 (latent 64^2)"))
        dt_name = {torch.float16: "f16", torch.bfloat16: "bf16"}[pipe.unet.dtype]
        line = {
            "metric": metric, "value": n_images / elapsed, "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dt_name, "data": "synthetic",
            "config": {"workload": f"W-{args.workload}: {shape}, {args.ddim_steps} DDIM steps, "
                                   f"meta_prompt '{rc.meta_prompt}', guidance 7.5, thresholds {rc.thresholds}, 1 seed per step",
                       "parallelism": f"seed-parallel x{world}", "guidance_forward": args.guidance_forward,
                       "skip_unused_guidance": args.skip_unused_guidance, "model": args.model,
                       "loss_only_steps": ("two passes (B=1 guidance, B=2 CFG)" if args.no_joint_pass or args.eager else
                                           "guidance forward + CFG pair of a step without latent update batched as one "
                                           "B=3 pass (every evaluation performed)"),
                       "launch": "eager" if args.eager else "hipGraph replay of the UNet passes (captured in warm-up)",
                       "refinement": ("enqueue, read the loss table, decide, enqueue" if args.eager or not pipe.speculative_refinement
                                      else "run-ahead: an iteration's backward, latent update and the next guidance evaluation "
                                           "are enqueued before its loss table is read (pinned asynchronous copy); same "
                                           "launches and counters; an enqueued update is discarded and repeated only on a "
                                           f"loss of exactly 0 — happened {pipe.discarded_speculations} times in this run, "
                                           "never counted in unet_calls"),
                       "weights": "seeded random init (no checkpoint offline)",
                       "amortised_outside_the_clock": "done once in the warm-up image(s), reused by every timed image (same "
                                                      "prompt, same 50 timesteps): hipGraph capture, packed conv weights, "
                                                      "the text K/V projections, the timestep-only part of the UNet (time "
                                                      "MLP + 22 per-block projections per timestep); initial latents and "
                                                      "the re-noise tensors are staged in HBM before the clock starts",
                       "roofline_method": "achieved = per-shape hipGraph micro-replay (100 launches between two HIP events "
                                          "on the launch stream, cold weights for the convolutions) weighted by the timed "
                                          "region's launch census; not an in-pipeline per-launch timing",
                       "side_effects": "PNG / log dumps of the reference (diagnostics) are off and outside the timed region"},
            "unet_calls_per_image": calls, "finite": ok,
            "weight_broadcast": bcast,
            "distributed": {"backend": dist.get_backend() if world > 1 else None, "world_size": world,
                            "self_launched": os.environ.get("GA_BENCH_SELF_LAUNCHED") == "1",
                            "images_per_s_per_rank": [round(x, 4) for x in per_rank],
                            "gathered_latents": sum(len(x) for x in gathered) if gathered else 0},
        }
        if two_pass is not None:
            line["two_pass_images_per_s"] = round(two_pass, 4)
        if first_image_s is not None:
            line["cold_first_image_s"] = round(first_image_s, 2)
        if flops_per_fwd:
            tf = flops_per_fwd * (calls["fwd_b1_grad"] + 2 * calls["fwd_b2"] + calls["bwd"]) / 1e12
            line["end_to_end"] = {"tflop_per_image": round(tf, 1),
                                  "achieved_tflops_per_gpu": round(tf * args.steps / elapsed, 1),
                                  "frac_of_2.5PF_dense_fp16": round(tf * args.steps / elapsed / 2500.0, 4)}
            # SURVEY's formula counts a backward as one full forward (0.803 TFLOP); the backward only covers the sub-graph below
            # the last 16 x 16 cross-attention map.  Beside it: the flops the captured passes really issue on the matrix cores,
            # from the launch census of each hipGraph (hand-written MFMA kernels only: the library's conv_in / conv_out / text
            # K/V GEMMs, < 1 % of a pass, are not in the census), times the run-time call counters.
            runner = getattr(pipe, "_runner", None)
            if runner is not None and not args.eager:
                per_pass = {name: sum(kernel_work(k)[1] * n for k, n in cen.items() if kernel_work(k)[0] == "mfma") / 1e12
                            for name, cen in runner.launches.items()}
                joint = calls.get("joint_b3", 0) if "joint" in per_pass else 0
                tf_c = (per_pass["eval"] * (calls["fwd_b1_grad"] - joint) + per_pass["grad"] * calls["bwd"] +
                        per_pass["cfg"] * (calls["fwd_b2"] - joint) + per_pass.get("joint", 0.0) * joint)
                line["end_to_end"].update({
                    "mfma_tflop_per_pass_from_census": {k: round(v, 3) for k, v in per_pass.items()},
                    "tflop_per_image_from_census": round(tf_c, 1),
                    "achieved_tflops_per_gpu_from_census": round(tf_c * args.steps / elapsed, 1),
                    "frac_of_2.5PF_from_census": round(tf_c * args.steps / elapsed / 2500.0, 4)})
        line["roofline"] = roof
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(args, cfg, calls, rc)
            line["speedup_vs_cpu_baseline"] = line["value"] / line["cpu_baseline"]["value"]
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if not ok:
        raise SystemExit("non-finite latents: the printed line is not a valid measurement")


if __name__ == "__main__":
    main()
