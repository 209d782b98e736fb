"""The guidance-step program (GuidedAttention._guidance_step / _perform_iterative_refinement_step) on the CPU, without a UNet:
a scripted driver answers its requests with hand-made loss parts and records them; the same scripted losses go through the
oracle's loop (oracle.pipeline.GuidedSampler with scripted _evaluate / _update and a stub UNet), which follows the reference's
control flow.  Both must do the same things in the same order and count the same calls."""
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import load_json
from guided_attention_amd import ops
from guided_attention_amd.pipeline_guided_attention import TERM, GuidedAttention
from guided_attention_amd.scheduler import DDIMScheduler
from guided_attention_amd.utils import helpers, shared_state as state
from oracle import loss as oloss
from oracle.pipeline import GuidedSampler

ENTRIES = [{"index": 2, "kind": "BOX", "geom": (.6, .3, .4, .55), "subprompt": "robot"},
           {"index": 5, "kind": "BOX", "geom": (.2, .3, .4, .55), "subprompt": "vase"}]
HIGH, LOW = (0.9, 0.8), (0.1, 0.2)      # unscaled losses per token: far above / far below every threshold used here (0.5)


def ev(unscaled, total=None):
    """One scripted evaluation: the per-token unscaled losses and the loss the `loss != 0` tests see (default: their sum)."""
    return (sum(unscaled) if total is None else total, tuple(unscaled))


def _mask_numbers(lines):
    return [re.sub(r"-?\d+(\.\d+)?(e-?\d+)?", "#", ln) for ln in lines]


def run_program(script, *, steps, thresholds, hyper, only_thr=True, max_iter_to_alter=25, run_standard_sd=False, guided=True,
                joint=False):
    """The product's program under a scripted driver -> what it did (events: evaluations, updates, CFG steps and re-noises in
    order), its call counters, the requests themselves (step index first), the re-noise coefficients and the masked log."""
    script = list(script)
    hp = dict(state.hyperParameterOverrides, **hyper)
    entries = ENTRIES if guided else []
    cfg = SimpleNamespace(
        token_dict={e["index"]: {"word": e["subprompt"], "subprompt": e["subprompt"], "loss_type": helpers.AnnotationType.BOX}
                    for e in entries},
        thresholds=dict(thresholds), only_update_on_threshold_steps=only_thr, sub_prompt_avg_within=False)
    plan = ops.LossPlan(entries, hp)
    pipe = GuidedAttention(unet=None)
    pipe.scheduler = DDIMScheduler()
    pipe.scheduler.set_timesteps(steps)
    im = pipe._image_record(cfg, hp, dict(thresholds), [], None, [], None, 0.0)

    def parts():
        total, unscaled = script.pop(0)
        terms = torch.zeros(len(entries), 8)
        terms[:, TERM["unscaled"]] = torch.tensor(unscaled)
        terms[:, TERM["token_loss"]] = torch.tensor(unscaled)
        loss = torch.tensor([float(total)])
        return terms, loss, None, plan, torch.cat([terms.reshape(-1), loss, torch.zeros(1)])

    events, requests, coefficients = [], [], []
    for i, t in enumerate(pipe.scheduler.timesteps):
        prog = pipe._guidance_step(i, int(t), im.thresholds, 20.0, max_iter_to_alter, run_standard_sd, joint)
        request = pipe._resume(im, prog, None, i)
        while request is not None:
            requests.append((i,) + request)
            kind, reply = request[0], None
            if kind in ("eval", "joint"):
                reply = parts()
                events += ["eval"] + ["cfg"] * (kind == "joint")
            elif kind == "update":
                assert request[2] is reply_loss, "the update request carries the loss _compute_loss returned"
                events.append("update")
                reply = torch.tensor(0.25)
            elif kind == "renoise":
                events.append("renoise")
                coefficients.append(request[1:])
            else:
                events.append({"fwd": "eval", "momentum": "momentum", "cfg": "cfg"}[kind])
            if kind == "eval":
                reply_loss = reply[1]
            request = pipe._resume(im, prog, reply, i)
    pipe._flush_image_logs(im)
    assert not script, "every scripted evaluation was asked for"
    return SimpleNamespace(events=events, calls=im.calls, requests=requests, coefficients=coefficients,
                           lines=_mask_numbers(im.lines))


class _StubUNet:
    """What GuidedSampler needs of a UNet when _evaluate is scripted: the CFG pass (zeros) and the processor hooks."""
    attn_processors = {}

    def __init__(self, events):
        self.events = events

    def set_attn_processor(self, procs):
        pass

    def __call__(self, x, t, encoder_hidden_states=None):
        self.events.append("cfg")
        return SimpleNamespace(sample=torch.zeros_like(x))


class _Noise:
    """A re-noise tensor that records being consumed: the oracle computes sqrt(1 - Bt) * noise."""

    def __init__(self, events, coefficients):
        self.events, self.coefficients = events, coefficients

    def __rmul__(self, coeff):
        self.events.append("renoise")
        self.coefficients.append(float(coeff))
        return torch.zeros(1, 4, 2, 2)


class _ScriptedSampler(GuidedSampler):
    def _evaluate(self, latents, t, cond):
        total, unscaled = self.script.pop(0)
        self.calls["fwd_b1_grad"] += 1
        self.calls["loss_evals"] += 1
        self.events.append("eval")
        return latents, {"loss": total}, oloss.subprompt_sums(self.plan, unscaled)

    def _update(self, latents, loss, step):
        self.calls["bwd"] += 1
        self.events.append("update")
        return latents


def run_oracle(script, *, steps, thresholds, hyper, only_thr=True, max_iter_to_alter=25, run_standard_sd=False):
    events, coefficients = [], []
    smp = _ScriptedSampler(_StubUNet(events), oloss.TokenPlan(ENTRIES, hyper), thresholds=thresholds,
                           only_update_on_threshold_steps=only_thr, max_iter_to_alter=max_iter_to_alter,
                           run_standard_sd=run_standard_sd, steps=steps)
    smp.script, smp.events = list(script), events
    smp.sample(torch.zeros(1, 4, 2, 2), torch.zeros(2, 77, 8), [_Noise(events, coefficients) for _ in range(16)])
    assert not smp.script
    return SimpleNamespace(events=events, calls=smp.calls, coefficients=coefficients, trace=smp.trace)


ONE_ROUND = {"recurse_steps": 1}
REFINE_3 = [ev(HIGH)] + [ev(HIGH), ev(HIGH), ev(LOW)] + [ev(LOW)]         # step evaluation, 3 iterations (met at the third), final
REFINE_CAP = [ev(HIGH)] + [ev(HIGH)] * 10 + [ev(HIGH)]                    # never met: the cap of 10, then the final evaluation
# name -> (scripted evaluations, arguments of both loops, what the program's counters must read)
SCENARIOS = {
    "threshold met at once": ([ev(LOW), ev(LOW)], dict(steps=2, thresholds={0: 0.5}, hyper=ONE_ROUND),
                              dict(fwd_b1_grad=2, bwd=0, fwd_b2=2)),
    "met after 3 iterations": (REFINE_3 + [ev(LOW)], dict(steps=2, thresholds={0: 0.5}, hyper=ONE_ROUND),
                               dict(fwd_b1_grad=6, bwd=4, fwd_b2=2)),     # 3 refinement updates + the pre-refinement test's (:999)
    "never met: the cap": (REFINE_CAP + [ev(LOW)], dict(steps=2, thresholds={0: 0.5}, hyper=ONE_ROUND),
                           dict(fwd_b1_grad=13, bwd=11, fwd_b2=2)),
    "a loss of exactly 0 in the refinement": ([ev(HIGH), ev(HIGH), ev(HIGH, total=0.0), ev(LOW), ev(LOW, total=0.0), ev(LOW)],
                                              dict(steps=2, thresholds={0: 0.5}, hyper=ONE_ROUND),
                                              dict(fwd_b1_grad=6, bwd=2, fwd_b2=2)),   # no update at iteration 2, none after the final
    # every step below max_iter_to_alter = 3 takes the pre-refinement test against the LAST threshold: step 0 after a
    # refinement that ended below it (fires: it reads the losses from before), step 1 passes, step 2 fires, step 3 is past
    "updates off the threshold steps": (REFINE_3 + [ev(LOW), ev(HIGH), ev(HIGH)],
                                        dict(steps=4, thresholds={0: 0.5}, hyper=ONE_ROUND, only_thr=False, max_iter_to_alter=3),
                                        dict(fwd_b1_grad=8, bwd=5, fwd_b2=4)),
    # step 0 recurses three rounds (two re-noises); step 2 lies past recurse_until = 1: one round
    "recurse cut off by recurse_until": (REFINE_3 * 3 + [ev(LOW)] + REFINE_3 + [ev(LOW)],
                                         dict(steps=4, thresholds={0: 0.5, 2: 0.5}, hyper={"recurse_steps": 3, "recurse_until": 1}),
                                         dict(fwd_b1_grad=22, bwd=16, fwd_b2=6)),
    # 2 steps: timesteps 501, 1; the step before t = 1 is <= 0: the rounds repeat without a re-noise
    "no re-noise at the last timestep": ([ev(LOW)] + REFINE_3 * 3,
                                         dict(steps=2, thresholds={1: 0.5}, hyper={"recurse_steps": 3, "recurse_until": 5}),
                                         dict(fwd_b1_grad=16, bwd=12, fwd_b2=4)),
    "run_standard_sd": ([ev(HIGH), ev(HIGH)], dict(steps=2, thresholds={0: 0.5}, hyper=ONE_ROUND, run_standard_sd=True),
                        dict(fwd_b1_grad=2, bwd=0, fwd_b2=2)),
}


def _named_updates_are_what_follows(requests):
    """Only the refinement's evaluations name an update, and what follows one is that update with the loss added, or — the loss
    was exactly 0 — the next evaluation.  -> how many evaluations named one."""
    named = 0
    for r, nxt in zip(requests, requests[1:]):
        if r[1] == "eval" and r[2] is not None:
            named += 1
            assert nxt[1] == "eval" or nxt[1:-1] == r[2], (r, nxt)
    return named


@pytest.mark.parametrize("name", SCENARIOS)
def test_program_does_what_the_oracle_loop_does(name):
    script, kw, expected = SCENARIOS[name]
    got, ref = run_program(script, **kw), run_oracle(script, **kw)
    assert got.events == ref.events
    assert {k: got.calls[k] for k in ref.calls} == ref.calls
    assert {k: got.calls[k] for k in expected} == expected and got.calls["joint_b3"] == 0
    assert got.coefficients == [(pytest.approx((1 - b * b) ** 0.5, rel=1e-5), pytest.approx(b, rel=1e-5)) for b in ref.coefficients]
    assert got.events.count("renoise") == (2 if "recurse" in name else 0)
    assert _named_updates_are_what_follows(got.requests) == sum(1 for e in ref.trace if e[0] == "refine")
    assert got.lines.count("gradient size average: #\n") == expected["bwd"]


def test_unguided_state_runs_the_forward_nobody_reads():
    """No annotated token: the reference's guidance forward has no consumer; it is asked for, and counted, but no loss is."""
    kw = dict(steps=3, thresholds={0: 0.5}, hyper=ONE_ROUND)
    got = run_program([], guided=False, **kw)
    assert [r[1:] for r in got.requests] == [("fwd",), ("cfg",)] * 3
    assert got.calls == {"fwd_b1_grad": 3, "bwd": 0, "fwd_b2": 3, "loss_evals": 0, "joint_b3": 0}
    ref = run_oracle([ev(LOW)] * 3, run_standard_sd=True, **kw)     # the oracle's closest form: evaluations nothing follows
    assert got.events == ref.events and {k: got.calls[k] for k in ("fwd_b1_grad", "bwd", "fwd_b2")} == \
        {k: ref.calls[k] for k in ("fwd_b1_grad", "bwd", "fwd_b2")}


def test_joint_steps_count_and_log_like_two_pass_steps():
    """Steps on which no update can follow are one ("joint",) request with a driver that serves it: same events and counters
    as the oracle, the loss lines — read at the end of the call — at the places the two-pass form logs them."""
    script = REFINE_3 + [ev(LOW), ev(HIGH)]
    kw = dict(steps=3, thresholds={0: 0.5}, hyper=ONE_ROUND)
    got, two_pass, ref = run_program(script, joint=True, **kw), run_program(script, **kw), run_oracle(script, **kw)
    assert [r[1] for r in got.requests if r[0] > 0] == ["joint", "joint"] and "joint" not in [r[1] for r in two_pass.requests]
    assert got.events == two_pass.events == ref.events
    assert got.calls == dict(two_pass.calls, joint_b3=2) and {k: got.calls[k] for k in ref.calls} == ref.calls
    assert got.lines == two_pass.lines


def test_momentum_refinement_steps_on_every_evaluation():
    """`use_optimizer` (no oracle counterpart): one ("momentum", lr, first, loss) per refinement evaluation, whatever the loss,
    `first` on the first evaluation of each refinement call only; the counters of tests/golden/g12_momentum.json."""
    meta = load_json("g12_momentum.json")[0]
    thr = {int(k): v for k, v in meta["thresholds"].items()}
    assert thr == {0: 2.5, 1: 0.5} and meta["steps"] == 5
    high = (3.0, 1.0)                                    # above both thresholds; an evaluation of exactly 0 is stepped on all the same
    script = [ev(high)] + [ev(high)] * 4 + [ev(high, total=0.0)] + [ev(high)] * 5 + [ev(high)] + REFINE_CAP + [ev(LOW)] * 3
    got = run_program(script, steps=5, thresholds=thr, hyper=meta["hyper"], max_iter_to_alter=meta["max_iter_to_alter"])
    momentum = [r for r in got.requests if r[1] == "momentum"]
    assert len(momentum) == meta["optimizer_steps"] == _named_updates_are_what_follows(got.requests)
    assert [r[3] for r in momentum] == ([True] + [False] * 9) * 2 and all(r[2] == 20.0 / 2.5 for r in momentum)
    assert [r[1] for r in got.requests].count("update") == meta["bwd"]          # the pre-refinement test's plain updates
    assert (got.calls["fwd_b1_grad"], got.calls["fwd_b2"]) == (meta["fwd_b1"], meta["fwd_b2"])
    assert got.calls["bwd"] == meta["optimizer_steps"] + meta["bwd"]
    assert "".join({"eval": "1", "cfg": "2"}.get(e, "") for e in got.events) == meta["call_sequence"]
    assert got.lines.count("\t Exceeded max number of iterations (#)! \n") == meta["exceeded_cap"]
    assert got.lines.count("gradient size average: #\n") == meta["bwd"]          # the momentum step logs none

