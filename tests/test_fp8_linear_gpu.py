"""ops.fp8_linear on the GPU: the three FP8 GEMMs' plumbing, checked per
element with the quantisation error excluded, the quantisation error itself
against the unquantised product, autograd behaviour, and a tiny Llama with
its projections converted.

Plumbing.  The fp64 references are built from the kernels' own e4m3 values
and inverse scales, (qx * isx) @ (qw * isw)^T and likewise for dX and dW, so
what remains is the GEMM's fp32 accumulation and the bf16 rounding of the
result: tests/utils_numerics.assert_bf16_close, 2^-8 |ref| + 2^-16 mag +
2^-126 with mag the product of the operands' absolute values.  A swapped
scale, a wrong transpose or a wrong layout is off by orders of magnitude.

Quantisation error.  Relative Frobenius error against the fp64 product of
the bf16 inputs: at most 0.05 where M*K >= 16384 (the eager CPU path measures
0.0367-0.0389 on these shapes and recipes over three seeds; a wrong operand
gives about 1.0), 0.06 at (16, 16, 16), where the small sample alone ranges
0.032-0.041."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import utils_numerics as N
from distributed_training_guide_amd.models.llama import (LlamaConfig,
                                                         LlamaForCausalLM)
from distributed_training_guide_amd.ops import (Fp8Linear,
                                                convert_linears_to_fp8,
                                                fp8_linear, fp8_quantize)

MKN = [(16, 16, 16), (64, 256, 128), (208, 80, 48), (128, 4096, 256)]
mkn = pytest.mark.parametrize("M,K,Nf", MKN,
                              ids=[f"M{m}-K{k}-N{n}" for m, k, n in MKN])


def _inputs(M, K, Nf):
    g = torch.Generator(device="cpu").manual_seed(M * 131 + K * 17 + Nf)
    x = torch.randn(M, K, generator=g).bfloat16().cuda()
    w = (0.02 * torch.randn(Nf, K, generator=g)).bfloat16().cuda()
    dy = torch.randn(M, Nf, generator=g).bfloat16().cuda()
    return x, w, dy


def _run(x, w, dy):
    x = x.clone().requires_grad_()
    w = w.clone().requires_grad_()
    y = fp8_linear(x, w)
    y.backward(dy)
    return y.detach(), x.grad, w.grad


@functools.lru_cache(maxsize=None)
def _case(M, K, Nf):
    x, w, dy = _inputs(M, K, Nf)
    y, dx, dw = _run(x, w, dy)

    def dequant(t):
        q, _, _, inv = fp8_quantize(t)
        return q.float().double() * inv.double()

    X, W, DY = dequant(x), dequant(w), dequant(dy)
    deq = dict(y=(X @ W.t(), X.abs() @ W.abs().t()),
               dx=(DY @ W, DY.abs() @ W.abs()),
               dw=(DY.t() @ X, DY.abs().t() @ X.abs()))
    xd, wd, dyd = x.double(), w.double(), dy.double()
    exact = dict(y=xd @ wd.t(), dx=dyd @ wd, dw=dyd.t() @ xd)
    torch.cuda.synchronize()
    return dict(x=x, w=w, dy=dy, out=dict(y=y, dx=dx, dw=dw), deq=deq,
                exact=exact)


@mkn
def test_gemm_plumbing_per_element(M, K, Nf):
    c = _case(M, K, Nf)
    shapes = dict(y=(M, Nf), dx=(M, K), dw=(Nf, K))
    for name in ("y", "dx", "dw"):
        got = c["out"][name]
        assert got.shape == shapes[name] and got.dtype == torch.bfloat16
        ref, mag = c["deq"][name]
        N.assert_bf16_close(got, ref, mag, what=f"{name} M{M} K{K} N{Nf}")


@mkn
def test_error_against_unquantised_product(M, K, Nf):
    c = _case(M, K, Nf)
    bound = 0.05 if M * K >= 16384 else 0.06
    errs = {}
    for name in ("y", "dx", "dw"):
        ref = c["exact"][name]
        errs[name] = ((c["out"][name].double() - ref).norm()
                      / ref.norm()).item()
    print(f"M{M} K{K} N{Nf} relative Frobenius error: {errs}")
    for name, err in errs.items():
        assert err <= bound, (name, err, bound)


@mkn
def test_second_run_is_bit_identical(M, K, Nf):
    c = _case(M, K, Nf)
    y, dx, dw = _run(c["x"], c["w"], c["dy"])
    for name, got in (("y", y), ("dx", dx), ("dw", dw)):
        assert torch.equal(got.view(torch.int16),
                           c["out"][name].view(torch.int16)), name


def test_autograd_grads_are_bf16_with_input_shapes():
    torch.manual_seed(0)
    lin = Fp8Linear(64, 48, bias=False, device="cuda", dtype=torch.bfloat16)
    x = torch.randn(2, 3, 16, 64, device="cuda").bfloat16().requires_grad_()
    y = lin(x)
    assert y.shape == (2, 3, 16, 48) and y.dtype == torch.bfloat16
    y.float().square().sum().backward()
    assert x.grad.dtype == torch.bfloat16 and x.grad.shape == x.shape
    assert lin.weight.grad.dtype == torch.bfloat16
    assert lin.weight.grad.shape == lin.weight.shape
    assert torch.isfinite(x.grad).all() and torch.isfinite(lin.weight.grad).all()
    # a frozen weight: only dX is produced
    lin.weight.grad = None
    lin.weight.requires_grad_(False)
    x.grad = None
    lin(x).float().sum().backward()
    assert x.grad is not None and lin.weight.grad is None


def test_dims_must_be_multiples_of_16():
    w = torch.randn(32, 32, device="cuda").bfloat16()
    with pytest.raises(ValueError, match="multiples of 16"):
        fp8_linear(torch.randn(24, 32, device="cuda").bfloat16(), w)
    with pytest.raises(ValueError, match="multiples of 16"):
        fp8_linear(torch.randn(32, 24, device="cuda").bfloat16(),
                   torch.randn(32, 24, device="cuda").bfloat16())
    with pytest.raises(ValueError, match="multiples of 16"):
        fp8_linear(torch.randn(32, 32, device="cuda").bfloat16(),
                   torch.randn(24, 32, device="cuda").bfloat16())
    with pytest.raises(TypeError, match="bf16"):
        fp8_linear(torch.randn(32, 32, device="cuda"), w)


# --------------------------------------------------------------------------
# tiny Llama
# --------------------------------------------------------------------------
TINY = dict(vocab_size=512, hidden_size=128, intermediate_size=256,
            num_hidden_layers=2, num_attention_heads=2,
            num_key_value_heads=2, max_position_embeddings=2048)
BATCH, SEQ = 2, 64
# One seed for every run below.  The bound on the GPU's fp8-vs-bf16 loss gap
# is twice the same gap of the eager CPU path on that seed.  The gap is a
# signed sum of small per-token perturbations and can cancel by chance: the
# CPU path gives 1.6e-4, 1.7e-3, 6.2e-4 and 1.5e-3 for seeds 0-3 (mean
# 1.0e-3).  Seed 1 is the first whose gap is not below that mean, so the
# bound is not set by a cancellation; it was fixed before any GPU run.
TINY_SEED = 1


@functools.lru_cache(maxsize=None)
def _tiny_llama():
    cfg = LlamaConfig(**TINY)
    torch.manual_seed(TINY_SEED)
    cpu = LlamaForCausalLM(cfg, device="cpu", dtype=torch.bfloat16)
    ids = torch.randint(0, TINY["vocab_size"], (BATCH, SEQ))
    out = {}
    for dev in ("cpu", "cuda"):
        model = copy.deepcopy(cpu).to(dev)
        keys = list(model.state_dict().keys())
        x = ids.to(dev)
        with torch.no_grad():
            bf16_loss = model(input_ids=x, labels=x).loss.float().item()
        names = convert_linears_to_fp8(model)
        loss = model(input_ids=x, labels=x).loss
        loss.backward()
        out[dev] = dict(model=model, keys=keys, names=names,
                        bf16_loss=bf16_loss, fp8_loss=loss.float().item())
    torch.cuda.synchronize()
    return out


def test_tiny_llama_conversion_keeps_state_dict():
    t = _tiny_llama()["cuda"]
    assert list(t["model"].state_dict().keys()) == t["keys"]
    want = [f"layers.{i}.{m}" for i in range(TINY["num_hidden_layers"])
            for m in ("self_attn.qkv_proj", "self_attn.o_proj",
                      "mlp.gate_up_proj", "mlp.down_proj")]
    assert t["names"] == want
    assert type(t["model"].lm_head) is torch.nn.Linear


def test_tiny_llama_loss_and_grads_finite():
    t = _tiny_llama()["cuda"]
    assert t["fp8_loss"] == t["fp8_loss"] and abs(t["fp8_loss"]) < 1e9
    for name, p in t["model"].named_parameters():
        assert p.grad is not None, name
        assert p.grad.dtype == torch.bfloat16 and p.grad.shape == p.shape
        assert torch.isfinite(p.grad).all(), name


def test_tiny_llama_initial_loss_close_to_bf16():
    t = _tiny_llama()
    cpu_gap = abs(t["cpu"]["fp8_loss"] - t["cpu"]["bf16_loss"])
    gpu_gap = abs(t["cuda"]["fp8_loss"] - t["cuda"]["bf16_loss"])
    print(f"bf16 loss cpu {t['cpu']['bf16_loss']:.6f} gpu "
          f"{t['cuda']['bf16_loss']:.6f}; fp8 loss cpu "
          f"{t['cpu']['fp8_loss']:.6f} gpu {t['cuda']['fp8_loss']:.6f}; "
          f"gap cpu {cpu_gap:.3e} gpu {gpu_gap:.3e}")
    assert cpu_gap > 0.0
    assert gpu_gap <= 2.0 * cpu_gap, (gpu_gap, cpu_gap)
