"""FP8 (OCP e4m3) linear layers: tensor-wise dynamic scaling around the
hipBLASLt FP8 GEMMs that `torch._scaled_mm` reaches.

The GEMMs stay with hipBLASLt; what this project adds is the memory-bound
work around them (fp8_quant.hip): one pass for a tensor's amax and scales,
one pass that scales, casts bf16 -> e4m3 and writes the row-major copy, the
transposed copy the backward GEMMs need, or both.  Activations, weights and
output gradients all use e4m3 with a scale computed from the tensor itself;
there is no scaling history and no e5m2.

    scale     = 448 / max(amax, 1e-12)          (fp32, IEEE division)
    inv_scale = max(amax, 1e-12) / 448          (its own division, not 1/scale)
    q         = rne(clamp(float(x) * scale, -448, 448))

An all-zero tensor quantises to zeros.  A non-finite input is not hidden: a
NaN gives NaN scales and an all-NaN result, an inf gives scale 0 and
inv_scale inf.

All three GEMMs of a linear use the form `_scaled_mm` wants, both operands
contiguous along the reduced dimension (A row-major, B column-major):

    fwd    Y  = Xq [M,K]  @ Wq [N,K]^T     * inv_sx  * inv_sw
    dgrad  dX = dYq [M,N] @ WqT [K,N]^T    * inv_sdy * inv_sw
    wgrad  dW = dYqT [N,M] @ XqT [K,M]^T   * inv_sdy * inv_sx

Saved for backward: XqT in fp8 (instead of the bf16 input autograd would
keep), three scales and the weight parameter itself; WqT is re-cast from the
weight in backward with the forward's scale, so no fp8 weight copy lives
between the two.  Neither direction synchronises the host.

CPU path (unit tests, the reference for the GPU tests): the same
quantisation in eager torch, then dequantise and multiply in fp32.
"""
import torch
import torch.nn as nn

from .._ext import ext, use_hip

E4M3_MAX = 448.0
AMAX_FLOOR = 1e-12
FP8 = torch.float8_e4m3fn


def _scales_ref(x):
    amax = x.abs().max().float().clamp(min=AMAX_FLOOR)
    # tensor / tensor: `448.0 / amax` is torch's reciprocal-then-multiply,
    # two roundings, and differs from the IEEE quotient in the last bit
    top = torch.full_like(amax, E4M3_MAX)
    return top / amax, amax / top


def _cast_ref(x, scale):
    # torch's own cast gives NaN above 448, hence the clamp
    return (x.float() * scale).clamp(-E4M3_MAX, E4M3_MAX).to(FP8)


def fp8_quantize(x, rowwise=True, transposed=False, scale=None):
    """Quantise bf16 `x` [R, C] (R and C multiples of 16) to e4m3.

    Returns (q, qt, scale, inv_scale): q [R, C] if `rowwise` else None, qt
    [C, R] (= q.t(), contiguous) if `transposed` else None, and the two
    0-dim fp32 scales on x's device.  With `scale` given (a 1-element fp32
    tensor) that scale is used, no amax is taken, and inv_scale is None: it
    is defined from the amax, not from the scale."""
    if x.dim() != 2:
        raise ValueError(f"fp8_quantize expects [R, C], got {tuple(x.shape)}")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"fp8_quantize expects bf16, got {x.dtype}")
    if not (rowwise or transposed):
        raise ValueError("fp8_quantize: ask for at least one output")
    if x.shape[0] % 16 or x.shape[1] % 16 or x.numel() == 0:
        raise ValueError("fp8_quantize requires R and C to be positive "
                         f"multiples of 16, got {tuple(x.shape)}")
    inv_scale = None
    if use_hip(x):
        if scale is None:
            scales = ext().fp8_amax_scale(x)
            scale, inv_scale = scales[0], scales[1]
        q, qt = ext().fp8_cast_transpose(x, scale, rowwise, transposed)
        return q, qt, scale, inv_scale
    if scale is None:
        scale, inv_scale = _scales_ref(x)
    q = _cast_ref(x, scale)
    qt = q.t().contiguous() if transposed else None
    return (q if rowwise else None), qt, scale, inv_scale


def _mm(a, b, inv_a, inv_b):
    """bf16 [P, Q] = (a [P, L] * inv_a) @ (b [Q, L] * inv_b)^T for row-major
    e4m3 a and b."""
    if a.is_cuda:
        return torch._scaled_mm(a, b.t(), scale_a=inv_a, scale_b=inv_b,
                                out_dtype=torch.bfloat16,
                                use_fast_accum=False)
    return ((a.float() * inv_a) @ (b.float() * inv_b).t()).bfloat16()


class _Fp8LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        xq, xqt, _, inv_sx = fp8_quantize(x, True, True)
        wq, _, sw, inv_sw = fp8_quantize(weight, True, False)
        ctx.save_for_backward(xqt, inv_sx, sw, inv_sw, weight)
        return _mm(xq, wq, inv_sx, inv_sw)

    @staticmethod
    def backward(ctx, dy):
        xqt, inv_sx, sw, inv_sw, weight = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad
        dyq, dyqt, _, inv_sdy = fp8_quantize(dy.contiguous(), need_dx,
                                             need_dw)
        dx = dw = None
        if need_dx:
            _, wqt, _, _ = fp8_quantize(weight.detach(), False, True,
                                        scale=sw)
            dx = _mm(dyq, wqt, inv_sdy, inv_sw)
        if need_dw:
            dw = _mm(dyqt, xqt, inv_sdy, inv_sx)
        return dx, dw


def fp8_linear(x, weight):
    """y = x @ weight^T with every GEMM (forward, dgrad, wgrad) in e4m3.
    x [..., K] and weight [N, K] are bf16; y [..., N] is bf16.  M (the
    product of x's leading dims), N and K must be multiples of 16."""
    if x.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16:
        raise TypeError("fp8_linear expects bf16 x and weight, got "
                        f"{x.dtype} and {weight.dtype}")
    if weight.dim() != 2 or x.dim() < 1 or x.shape[-1] != weight.shape[1]:
        raise ValueError(f"fp8_linear: x {tuple(x.shape)} does not match "
                         f"weight {tuple(weight.shape)}")
    N, K = weight.shape
    M = x.numel() // K if K else 0
    if M % 16 or N % 16 or K % 16 or 0 in (M, N, K):
        raise ValueError("fp8_linear requires M, N and K to be positive "
                         f"multiples of 16, got M={M}, N={N}, K={K}")
    y = _Fp8LinearFn.apply(x.reshape(M, K).contiguous(), weight.contiguous())
    return y.view(*x.shape[:-1], N)


class Fp8Linear(nn.Linear):
    """nn.Linear (bias-free) whose three GEMMs run in e4m3.  Same parameters
    and state_dict as nn.Linear: only `forward` differs."""

    def forward(self, x):
        if self.bias is not None:
            raise ValueError("Fp8Linear supports bias-free linears only")
        return fp8_linear(x, self.weight)


def convert_linears_to_fp8(model, skip=("lm_head",)):
    """Turn the model's eligible nn.Linear modules into Fp8Linear in place
    (the class is swapped, nothing else: parameters, names, state_dict keys
    and optimizer state are untouched, checkpoints stay interchangeable with
    bf16 runs).  Eligible: exactly nn.Linear, no bias, in and out features
    multiples of 16, no component of its name in `skip`.  Returns the names
    converted."""
    converted = []
    for name, m in model.named_modules():
        if type(m) is not nn.Linear or m.bias is not None:
            continue
        if m.in_features % 16 or m.out_features % 16:
            continue
        if any(part in skip for part in name.split(".")):
            continue
        m.__class__ = Fp8Linear
        converted.append(name)
    return converted
