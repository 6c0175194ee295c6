"""GPT-2 HIP op numerics vs plain PyTorch fp32 references: LayerNorm
fwd/bwd (incl. dw/db reductions; norm.hip) and tanh-GELU fwd/bwd (gelu.hip)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rows,H", [
    (512, 768), (1000, 1600), (64, 104),
    (3, 100),    # H % 8 != 0: scalar path
    (2100, 64),  # > 2048 rows: a block folds two rows into one partial
    (5, 2056),   # two register chunks, the second is one thread's 8 columns
    (3, 4104),   # NCH = 4: chunk 3 is one thread, chunk 4 is empty
    (2, 8192),   # last H on the vector path, all four chunks full
    (2, 8200),   # H > 8192: past the register accumulators, scalar fallback
])
def test_layernorm_matches_fp32(rows, H):
    from distributed_training_guide_amd.ops.layernorm import LayerNorm

    torch.manual_seed(0)
    x = (torch.randn(4, rows // 4 if rows % 4 == 0 else rows, H,
                     device="cuda") * 2).bfloat16()
    if rows % 4 != 0:
        x = x[:1]
    ln = LayerNorm(H, eps=1e-5, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        ln.weight.normal_(1.0, 0.1)
        ln.bias.normal_(0.0, 0.1)

    xg = x.clone().requires_grad_(True)
    y = ln(xg)
    dy = torch.randn_like(y) * 0.5
    y.backward(dy)

    xf = x.float().requires_grad_(True)
    wf = ln.weight.detach().float().requires_grad_(True)
    bf = ln.bias.detach().float().requires_grad_(True)
    yf = torch.nn.functional.layer_norm(xf, (H,), wf, bf, 1e-5)
    yf.backward(dy.float())

    assert torch.allclose(y.float(), yf, atol=5e-2, rtol=2e-2), \
        (y.float() - yf).abs().max()
    assert torch.allclose(xg.grad.float(), xf.grad, atol=5e-2, rtol=5e-2), \
        (xg.grad.float() - xf.grad).abs().max()
    # reductions over many rows in bf16 out: coarser tolerance
    assert torch.allclose(ln.weight.grad.float(), wf.grad, atol=0.5,
                          rtol=2e-2), \
        (ln.weight.grad.float() - wf.grad).abs().max()
    assert torch.allclose(ln.bias.grad.float(), bf.grad, atol=0.5,
                          rtol=2e-2), \
        (ln.bias.grad.float() - bf.grad).abs().max()


def test_gelu_matches_fp32():
    from distributed_training_guide_amd.ops.layernorm import gelu

    torch.manual_seed(1)
    x = (torch.randn(1024, 3072, device="cuda") * 3).bfloat16()
    xg = x.clone().requires_grad_(True)
    y = gelu(xg)
    dy = torch.randn_like(y)
    y.backward(dy)

    xf = x.float().requires_grad_(True)
    yf = torch.nn.functional.gelu(xf, approximate="tanh")
    yf.backward(dy.float())

    assert torch.allclose(y.float(), yf, atol=2e-2, rtol=2e-2)
    assert torch.allclose(xg.grad.float(), xf.grad, atol=3e-2, rtol=3e-2), \
        (xg.grad.float() - xf.grad).abs().max()


def test_gpt2_fully_native_step():
    """GPT-2 trains through LN/GELU/attention/fused-CE HIP kernels and the
    GPU loss matches the CPU fp32 reference path."""
    from distributed_training_guide_amd.models import build_model
    from distributed_training_guide_amd.ops import FusedAdamW

    torch.manual_seed(0)
    m = build_model("gpt2", device=torch.device("cuda"),
                    dtype=torch.bfloat16)
    cpu = build_model("gpt2", device=torch.device("cpu"),
                      dtype=torch.float32)
    cpu.load_state_dict({k: v.float().cpu()
                         for k, v in m.state_dict().items()})
    ids = torch.randint(0, 50000, (2, 128), device="cuda")
    out = m(input_ids=ids, labels=ids)
    assert out.logits is None  # fused CE path taken
    ref = cpu(input_ids=ids.cpu(), labels=ids.cpu())
    rel = abs(out.loss.item() - ref.loss.item()) / ref.loss.item()
    assert rel < 3e-2, (out.loss.item(), ref.loss.item())
    opt = FusedAdamW(m.parameters(), lr=1e-4)
    out.loss.backward()
    opt.step()
    torch.cuda.synchronize()
