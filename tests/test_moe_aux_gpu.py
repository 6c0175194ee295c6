"""moe_router_aux.hip on the GPU: routing outputs bit-equal to the plain
router's, exact counts, both losses and every element of dlogits against the
fp64 definitions (tests/utils_moe_aux.py), run-to-run equality, and the
losses' way into a model's loss."""
import dataclasses

import pytest
import torch

from distributed_training_guide_amd._ext import ext
from distributed_training_guide_amd.models import build_model, get_config
from distributed_training_guide_amd.ops import moe_router
from utils_moe import router_logits
from utils_moe_aux import AUX_SHAPES, assert_aux_close, aux_ref64

pytestmark = pytest.mark.gpu


def _run(logits, k, norm, dw, g_aux, g_z):
    """(idx, w, aux, z, dlogits); dw None leaves topk_w without a gradient."""
    x = logits.clone().requires_grad_()
    idx, w, aux, z = moe_router(x, k, norm, aux=True)
    loss = g_aux * aux + g_z * z
    (loss if dw is None else loss + (w * dw).sum()).backward()
    return idx, w.detach(), aux.detach(), z.detach(), x.grad


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("recipe", ["plain", "masked"])
@pytest.mark.parametrize("shape", AUX_SHAPES)
def test_router_aux_matches_fp64(shape, recipe, norm):
    T, E, k = shape
    what = f"{shape} {recipe} norm={norm}"
    logits, dw = router_logits(T, E, k, recipe, "cuda")
    idx0, w0 = moe_router(logits, k, norm)
    counts = ext().moe_router_aux_fwd(logits, k, norm)[2]
    # with a gradient into topk_w, then without one, so that the aux terms
    # are not hidden below the rounding of the routing term
    for grads in ((dw, 1.5, -0.75), (None, 1.5, -0.75)):
        first = _run(logits, k, norm, *grads)
        idx, w, aux, z, dlogits = first
        assert torch.equal(idx, idx0) and torch.equal(w, w0), what
        ref = aux_ref64(logits, k, norm, torch.zeros_like(dw)
                        if grads[0] is None else dw, *grads[1:])
        assert torch.equal(counts.cpu(), ref["counts"]), what
        if recipe == "masked":
            assert counts[1].item() == 0
        assert_aux_close(aux, z, dlogits, ref, what)
        for a, b in zip(first, _run(logits, k, norm, *grads)):
            assert torch.equal(a, b), what


def test_model_loss_carries_the_router_losses():
    """out.loss is the coefficient-0 loss plus coef * mean(aux) +
    coef * mean(z) (two f32 adds: 2^-22 relative), and the router weights
    see the extra gradient."""
    cfg0 = get_config("qwen3-moe-debug")
    cfg1 = dataclasses.replace(cfg0, router_aux_loss_coef=0.01,
                               router_z_loss_coef=0.01)
    ids = torch.randint(0, cfg0.vocab_size, (2, 64),
                        generator=torch.Generator().manual_seed(0)).cuda()
    outs, grads = [], []
    for cfg in (cfg0, cfg1):
        torch.manual_seed(0)
        model = build_model(cfg, device="cuda", dtype=torch.bfloat16)
        outs.append(model(input_ids=ids, labels=ids))
        outs[-1].loss.backward()
        grads.append(model.layers[0].mlp.router.weight.grad)
    assert outs[0].router_aux_loss is None and outs[0].router_z_loss is None
    aux, z = outs[1].router_aux_loss, outs[1].router_z_loss
    assert aux.dim() == 0 and z.dim() == 0 and aux > 0 and z > 0
    torch.testing.assert_close(outs[1].loss, outs[0].loss + 0.01 * aux
                               + 0.01 * z, rtol=2.0 ** -22, atol=0.0)
    assert not torch.equal(grads[0], grads[1])
