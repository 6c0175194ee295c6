"""FP8 (OCP e4m3) linear layers: tensor-wise scaling around the hipBLASLt
FP8 GEMMs that `torch._scaled_mm` reaches.

The GEMMs stay with hipBLASLt; what this project adds is the memory-bound
work around them.  Activations, weights and output gradients all use e4m3
(no e5m2), with one of two recipes for the scale:

  dynamic (the default, fp8_quant.hip): the scale comes from the tensor
    itself.  One pass for its amax and scales, one pass that scales, casts
    bf16 -> e4m3 and writes the row-major copy, the transposed copy the
    backward GEMMs need, or both.
  delayed (fp8_delayed.hip, `Fp8DelayedState`): the scale comes from the
    amaxes of the last `history` quantisations of the same role (x, w or dy
    of one linear), so it is known before the tensor is read: one pass casts
    and records this call's amax, and SwiGLU can write e4m3 directly
    (`fp8_swiglu_linear`) so that the down projection's input never exists in
    bf16.  The first quantisation of a role runs the dynamic path and fills
    the history with its amax: no call casts with a made-up scale.

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
from .swiglu import silu_mul

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


def _history_update_ref(history, slot, amax):
    """fp8_history_update_kernel in eager torch: `amax` (0-dim fp32) into
    history[slot] in place (slot < 0, or a non-finite history: into every
    slot), a non-finite amax replaced by the previous max(history); returns
    the (scale, inv_scale) of max(history)."""
    prev = history.max()
    finite = bool(torch.isfinite(amax))
    if slot < 0 or not bool(torch.isfinite(prev)):
        history.fill_(amax if finite else float("nan"))
    else:
        history[slot] = amax if finite else prev
    a = history.max().clamp(min=AMAX_FLOOR)
    top = torch.full_like(a, E4M3_MAX)
    return top / a, a / top


class _Role:
    __slots__ = ("history", "pair", "count", "seeded")


class Fp8DelayedState:
    """Delayed scaling for the three operands (roles `x`, `w`, `dy`) of one
    linear: per role an fp32 `amax_history` [history] on the device, the
    current (scale, inv_scale) pair, and on the host a slot counter and a
    `seeded` flag.

    A plain object, not a module buffer: state_dict and checkpoints stay
    interchangeable with bf16 and dynamic-FP8 runs, and after a resume every
    role seeds again.  Created lazily on the first tensor's device.

    The first quantisation of a role runs the dynamic path (amax pass, then
    the cast) and fills the whole history with that amax.  Every later one
    casts with the current pair in one pass (fp8_cast_amax / silu_mul_fp8),
    writes the pass's amax into the next slot and rebinds the pair to a fresh
    tensor computed from max(history); the old pair stays valid for the GEMMs
    and the backward that hold it.  A non-finite amax does not enter the
    history (the slot repeats the previous max), though that call's output is
    NaN wherever its input was.

    The history advances once per quantisation call, not per optimizer
    step: under gradient accumulation or activation recomputation it
    advances several times a step.  It is per rank; there is no collective.
    Nothing here synchronises the host."""

    ROLES = ("x", "w", "dy")

    def __init__(self, history=16):
        if not 1 <= int(history) <= 1024:
            raise ValueError(f"amax history must be in [1, 1024], "
                             f"got {history}")
        self.history = int(history)
        self._roles = {}

    def role(self, name, device=None):
        """The role's record (history, pair, count, seeded); created on
        `device` at first use."""
        if name not in self.ROLES:
            raise ValueError(f"role must be one of {self.ROLES}, got {name!r}")
        r = self._roles.get(name)
        if r is None:
            r = self._roles[name] = _Role()
            r.history = torch.zeros(self.history, dtype=torch.float32,
                                    device=device)
            r.pair, r.count, r.seeded = None, 0, False
        return r

    def _advance(self, r, amax):
        # amax: the kernels' int32 tile partials, or a 0-dim fp32 tensor
        slot = r.count % self.history if r.seeded else -1
        if amax.dtype == torch.int32:
            pair = ext().fp8_history_update(amax, r.history, slot)
            r.pair = (pair[0], pair[1])
        else:
            r.pair = _history_update_ref(r.history, slot, amax)
        r.count += r.seeded
        r.seeded = True

    def quantize(self, x, role, rowwise=True, transposed=False):
        """fp8_quantize(x, rowwise, transposed, state=self, role=role)."""
        r = self.role(role, x.device)
        hip = use_hip(x)
        if r.seeded:
            scale, inv_scale = r.pair
        elif hip:
            scales = ext().fp8_amax_scale(x)
            scale, inv_scale = scales[0], scales[1]
        else:
            scale, inv_scale = _scales_ref(x)
        if hip:
            q, qt, amax = ext().fp8_cast_amax(x, scale, rowwise, transposed)
        else:
            q = _cast_ref(x, scale)
            qt = q.t().contiguous() if transposed else None
            q = q if rowwise else None
            amax = x.abs().max().float()
        self._advance(r, amax)
        return q, qt, scale, inv_scale

    def swiglu(self, gate_up):
        """Role `x` from the packed gate|up [R, 2I]: (hq [R, I], hqt [I, R],
        scale, inv_scale, path) of h = silu(gate) * up.  path is "fused"
        when silu_mul_fp8 wrote e4m3 directly, "seed" for the role's first
        call, which needs h's own amax before it can cast."""
        r = self.role("x", gate_up.device)
        if not (r.seeded and use_hip(gate_up)):
            path = "eager" if r.seeded else "seed"
            return (*self.quantize(silu_mul(gate_up), "x", True, True), path)
        scale, inv_scale = r.pair
        hq, hqt, amax = ext().silu_mul_fp8(gate_up, scale)
        self._advance(r, amax)
        return hq, hqt, scale, inv_scale, "fused"


def fp8_quantize(x, rowwise=True, transposed=False, scale=None, state=None,
                 role=None):
    """Quantise bf16 `x` [R, C] (R and C multiples of 16) to e4m3.

    Returns (q, qt, scale, inv_scale): q [R, C] if `rowwise` else None, qt
    [C, R] (= q.t(), contiguous) if `transposed` else None, and the two
    0-dim fp32 scales on x's device.  With `scale` given (a 1-element fp32
    tensor) that scale is used, no amax is taken, and inv_scale is None: it
    is defined from the amax, not from the scale.  With `state` (an
    Fp8DelayedState) and `role` the role's current scale is used, the
    inv_scale returned is the one that matches it, and the role's history
    advances by this tensor's amax (see Fp8DelayedState)."""
    if state is not None and (scale is not None or role is None):
        raise ValueError("fp8_quantize: `state` needs a `role` and excludes "
                         "`scale`")
    if x.dim() != 2:
        raise ValueError(f"fp8_quantize expects [R, C], got {tuple(x.shape)}")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"fp8_quantize expects bf16, got {x.dtype}")
    if not (rowwise or transposed):
        raise ValueError("fp8_quantize: ask for at least one output")
    if x.shape[0] % 16 or x.shape[1] % 16 or x.numel() == 0:
        raise ValueError("fp8_quantize requires R and C to be positive "
                         f"multiples of 16, got {tuple(x.shape)}")
    if state is not None:
        return state.quantize(x, role, rowwise, transposed)
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
    def forward(ctx, x, weight, state=None):
        xq, xqt, _, inv_sx = fp8_quantize(x, True, True, state=state,
                                          role="x")
        wq, _, sw, inv_sw = fp8_quantize(weight, True, False, state=state,
                                         role="w")
        ctx.state = state
        ctx.save_for_backward(xqt, inv_sx, sw, inv_sw, weight)
        return _mm(xq, wq, inv_sx, inv_sw)

    @staticmethod
    def backward(ctx, dy):
        xqt, inv_sx, sw, inv_sw, weight = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[:2]
        dyq, dyqt, _, inv_sdy = fp8_quantize(dy.contiguous(), need_dx,
                                             need_dw, state=ctx.state,
                                             role="dy")
        dx = dw = None
        if need_dx:
            _, wqt, _, _ = fp8_quantize(weight.detach(), False, True,
                                        scale=sw)
            dx = _mm(dyq, wqt, inv_sdy, inv_sw)
        if need_dw:
            dw = _mm(dyqt, xqt, inv_sdy, inv_sx)
        return dx, dw, None


def fp8_linear(x, weight, state=None):
    """y = x @ weight^T with every GEMM (forward, dgrad, wgrad) in e4m3.
    x [..., K] and weight [N, K] are bf16; y [..., N] is bf16.  M (the
    product of x's leading dims), N and K must be multiples of 16.  `state`
    (an Fp8DelayedState of this linear) selects delayed scaling; without it
    every scale is the tensor's own."""
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
    y = _Fp8LinearFn.apply(x.reshape(M, K).contiguous(), weight.contiguous(),
                           state)
    return y.view(*x.shape[:-1], N)


def _silu_mul_bwd(dh, gate_up):
    if use_hip(gate_up):
        return ext().silu_mul_bwd(dh.contiguous(), gate_up)
    with torch.enable_grad():
        gu = gate_up.detach().requires_grad_()
        return torch.autograd.grad(silu_mul(gu), gu, dh)[0]


# "fused" when the last fp8_swiglu_linear forward wrote e4m3 straight from
# the SwiGLU kernel, "seed" when it was the state's first call (which runs
# silu_mul and the dynamic path), "eager" on the CPU
last_swiglu_path = None


class _Fp8SwigluLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate_up, weight, state):
        global last_swiglu_path
        hq, hqt, _, inv_sh, last_swiglu_path = state.swiglu(gate_up)
        wq, _, sw, inv_sw = state.quantize(weight, "w", True, False)
        ctx.state = state
        ctx.save_for_backward(gate_up, hqt, inv_sh, sw, inv_sw, weight)
        return _mm(hq, wq, inv_sh, inv_sw)

    @staticmethod
    def backward(ctx, dy):
        gate_up, hqt, inv_sh, sw, inv_sw, weight = ctx.saved_tensors
        need_dgu, need_dw = ctx.needs_input_grad[:2]
        dyq, dyqt, _, inv_sdy = ctx.state.quantize(dy.contiguous(), "dy",
                                                   need_dgu, need_dw)
        dgu = dw = None
        if need_dgu:
            _, wqt, _, _ = fp8_quantize(weight.detach(), False, True,
                                        scale=sw)
            dgu = _silu_mul_bwd(_mm(dyq, wqt, inv_sdy, inv_sw), gate_up)
        if need_dw:
            dw = _mm(dyqt, hqt, inv_sdy, inv_sh)
        return dgu, dw, None


def fp8_swiglu_linear(gate_up, weight, state):
    """y = (silu(gate) * up) @ weight^T for the packed gate_up [..., 2I] and
    weight [N, I], both bf16, under delayed scaling (`state`, the down
    projection's Fp8DelayedState): the SwiGLU kernel writes its result as
    e4m3, row-major for the forward GEMM and transposed for wgrad, so h is
    never stored in bf16.  Equal bit for bit to
    fp8_linear(silu_mul(gate_up), weight, state).  Backward: dy is quantised,
    dgrad gives dh, wgrad takes the saved transposed h, and dgate_up is
    silu_mul's backward of dh on the saved gate_up.  M, N and I must be
    multiples of 16."""
    if gate_up.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16:
        raise TypeError("fp8_swiglu_linear expects bf16 gate_up and weight, "
                        f"got {gate_up.dtype} and {weight.dtype}")
    if not isinstance(state, Fp8DelayedState):
        raise TypeError("fp8_swiglu_linear needs an Fp8DelayedState")
    if (weight.dim() != 2 or gate_up.dim() < 1
            or gate_up.shape[-1] != 2 * weight.shape[1]):
        raise ValueError(f"fp8_swiglu_linear: gate_up {tuple(gate_up.shape)} "
                         f"does not match weight {tuple(weight.shape)}")
    N, I = weight.shape
    M = gate_up.numel() // (2 * I) if I else 0
    if M % 16 or N % 16 or I % 16 or 0 in (M, N, I):
        raise ValueError("fp8_swiglu_linear requires M, N and I to be "
                         f"positive multiples of 16, got M={M}, N={N}, I={I}")
    y = _Fp8SwigluLinearFn.apply(gate_up.reshape(M, 2 * I).contiguous(),
                                 weight.contiguous(), state)
    return y.view(*gate_up.shape[:-1], N)


class Fp8Linear(nn.Linear):
    """nn.Linear (bias-free) whose three GEMMs run in e4m3.  Same parameters
    and state_dict as nn.Linear: only `forward` differs.  `fp8_state` (an
    Fp8DelayedState, a plain attribute) selects delayed scaling."""

    fp8_state = None

    def forward(self, x):
        if self.bias is not None:
            raise ValueError("Fp8Linear supports bias-free linears only")
        return fp8_linear(x, self.weight, self.fp8_state)


def convert_linears_to_fp8(model, skip=("lm_head", "router"),
                           recipe="dynamic", history=16):
    """Turn the model's eligible nn.Linear modules into Fp8Linear in place
    (the class is swapped, nothing else: parameters, names, state_dict keys
    and optimizer state are untouched, checkpoints stay interchangeable with
    bf16 runs).  Eligible: exactly nn.Linear, no bias, in and out features
    multiples of 16, no component of its name in `skip`.  recipe="delayed"
    gives each converted module an Fp8DelayedState of `history` amaxes per
    role.  Returns the names converted."""
    if recipe not in ("dynamic", "delayed"):
        raise ValueError(f"recipe must be 'dynamic' or 'delayed', "
                         f"got {recipe!r}")
    converted = []
    for name, m in model.named_modules():
        if type(m) is not nn.Linear or m.bias is not None:
            continue
        if m.in_features % 16 or m.out_features % 16:
            continue
        if any(part in skip for part in name.split(".")):
            continue
        m.__class__ = Fp8Linear
        if recipe == "delayed":
            m.fp8_state = Fp8DelayedState(history)
        converted.append(name)
    return converted
