"""The four fused forms of the aggregate + loss (solo, S seeds of one prompt, S images of an ImageTable, the table with relation
rows) through autograd: AttnCapture -> the form's Function -> torch.autograd.grad back to q.  What is under test is the host
plumbing they share (ops._loss_fwd / _loss_bwd / _FusedLoss): that each image's dLoss/dA map reaches the capture backward as
that image's map (the image-broadcast hand-off), not as image 0's.  test_batched_loss_backward_reaches_the_capture_kernel of
test_output_bounds_gpu.py, for every form.

Shapes: S = 3 images (1 for the solo form), 2 heads, Kt = 77, D = 8, two guided tokens; res 5 (25 pixels: a ragged map, nothing is
staged) in f16 and bf16, res 16 in f16.  Per-image weights 1.5, 0, 0.75 (the solo form: 1.5; it has no second image to switch off).
"""
import pytest
import torch

from oracle import loss as oloss
from test_kernels_gpu import DT, TOL, close, make_qkv

pytestmark = pytest.mark.gpu

H, KT, D = 2, 77, 8
ENTRIES = [{"index": 2, "kind": "BOX", "geom": (.6, .3, .4, .55), "subprompt": "robot"},
           {"index": 5, "kind": "BOX", "geom": (.2, .3, .4, .55), "subprompt": "blue vase"}]
FORMS = ["solo", "batched", "images", "relation"]
CASES = [(5, "f16"), (5, "bf16"), (16, "f16")]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    _ops.prepare_device("cuda")
    return _ops


def _form(ops, form, res):
    """-> (images, Function(p) -> outputs, forward wrapper(p) -> outputs, backward wrapper(A, dloss, dtype) -> (dA, dP_bcast))."""
    plan = ops.LossPlan(ENTRIES, oloss.DEFAULT_HYPER)
    args = (res, 1, KT - 1, plan)
    if form == "solo":
        return (1, lambda p: ops.AggregateSmoothLoss.apply(*args, p), lambda p: ops.aggregate_loss_fwd([p], *args),
                lambda A, w, T: ops.smooth_loss_bwd(A, *args, w, T, 1.0 / H))
    S = 3
    if form == "batched":
        return (S, lambda p: ops.AggregateSmoothLossBatched.apply(S, *args, p),
                lambda p: ops.aggregate_loss_fwd_batched([p], S, *args),
                lambda A, w, T: ops.smooth_loss_bwd_batched(A, *args, w, T, 1.0 / H))
    rel = form == "relation"
    table = ops.ImageTable(S, 4, res, True, .5, 3, torch.device("cuda"), Q_max=4 if rel else 0)
    table.set([plan] * S, [(1, KT - 1)] * S, [ops.RelationPlan([([1], [4])]), None, None] if rel else None)
    if rel:
        return (S, lambda p: ops.AggregateSmoothLossRelImages.apply(table, p),
                lambda p: ops.aggregate_loss_rel_fwd_images([p], table),
                lambda A, w, T: ops.smooth_loss_rel_bwd_images(A, table, w, T, 1.0 / H))
    return (S, lambda p: ops.AggregateSmoothLossImages.apply(table, p), lambda p: ops.aggregate_loss_fwd_images([p], table),
            lambda A, w, T: ops.smooth_loss_bwd_images(A, table, w, T, 1.0 / H))


@pytest.mark.parametrize("res,dt", CASES, ids=[f"res{r}-{d}" for r, d in CASES])
@pytest.mark.parametrize("form", FORMS)
def test_loss_function_backward_reaches_the_capture_kernel(ops, form, res, dt):
    S, function, forward, backward = _form(ops, form, res)
    N, T, scale = res * res, DT[dt], D ** -0.5
    q, k, v = make_qkv(S, H, N, KT, D, T, 900 + res, 0.5)
    w = torch.tensor([1.5, 0.0, 0.75][:S], device="cuda")
    qa = q.clone().requires_grad_(True)
    o, p = ops.AttnCapture.apply(qa, k, v, H, scale, True)
    out = function(p)
    loss = out[-1]

    # the Function's forward is the wrapper's launch (deterministic); behind a relation form, total = box + relation loss
    ref_out = forward(p.detach())
    assert len(out) == len(ref_out) + (form == "relation") and loss.shape == (S,)
    for i, (got, ref) in enumerate(zip(out, ref_out)):
        assert torch.equal(got, ref), f"forward output {i}"
    if form == "relation":
        assert torch.equal(loss, out[2] + out[4])
        assert float(out[4][0]) > 0 and not out[4][1:].any()   # image 0 alone has a relation (near-equal centroids: v ~ 1.8)
    assert loss.requires_grad and not any(t.requires_grad for t in out[:-1])

    # no gradient for the loss: no launch, None for every input
    node = loss.grad_fn
    with ops.census_scope() as census:
        grads = node._forward_cls.backward(node, *([None] * len(out)))
    assert len(grads) == 2 and all(g is None for g in grads) and not census.launches

    ops.end_image_broadcasts()
    sentinel = [1, 1, None, 0]          # an entry of some earlier backward: only a form with images may clear the registry
    ops._image_broadcasts[0] = sentinel
    try:
        (dq,) = torch.autograd.grad((w * loss).sum(), [qa])
        A = out[0]
        dA, dPb = backward(A, w, T)
        if form == "solo":
            assert ops._image_broadcasts == {0: sentinel}
        else:
            (entry,) = ops._image_broadcasts.values()      # the one hand-off: S images, one map each, consumed by the one stored map
            assert entry[:2] == [S, N * KT] and entry[3] == 0 and torch.equal(entry[2], dPb)
            assert not entry[2][1].any() and not dq[1].any()        # weight 0: an exactly zero map, and nothing for its q
    finally:
        ops._image_broadcasts.pop(0, None)
    ops.end_image_broadcasts()

    dense = dPb.reshape(S, 1, N, KT).expand(S, H, N, KT).reshape(S * H, N, KT).contiguous()
    ref = ops.attn_capture_bwd(q, k, v, torch.zeros_like(q), dense, H, scale)
    assert all(float(ref[s].abs().max()) > 0 for s in range(S) if float(w[s]) != 0)
    close(dq, ref.double().cpu().numpy(), TOL[dt], f"{form}: strided entry vs the dense one")
    assert ops.tickets_are_zero()
