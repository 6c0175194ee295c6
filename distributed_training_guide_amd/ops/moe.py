"""Mixture-of-experts ops: fused top-k router (moe_router.hip), the
expert-sorted token layout and its row movers (moe_dispatch.hip) on GPU,
eager torch on CPU.

The rule of ops/fp8_linear.py holds here too: the GEMMs stay with the vendor
library (the router projection is a plain matmul, the expert GEMMs are
torch's grouped GEMM with device-side group offsets), and the memory-bound
work around them is hand-written HIP: softmax -> top-k -> renormalise, the
expert-sorted layout, the row scatter into it and the k-way weighted combine
back, each with its backward.  No host sync, no atomics (so no
non-deterministic index_add_), no cleared buffers.  The expert GEMMs have a
hand-written alternative as well, opt-in: expert_mm(impl="hip") /
moe_mlp(expert_gemm="hip") run the grouped bf16 MFMA GEMMs of moe_gemm.hip,
forward and backward; "hip-gather" also drops the scattered copy of the
tokens, the gate_up GEMM reading them through a row index
(moe_gemm_gather.hip); "hip-fused" also moves the activation into the GEMMs'
epilogues as a weighted SwiGLU (moe_gemm_swiglu.hip): the gate_up GEMM
writes h' = w * silu(g) * u beside gu, w the row's router weight, so the
combine is an unweighted k-way sum that saves nothing but dest, and the down
GEMM's dA turns into d gate_up-output and the router-weight gradient while
dh is still in accumulators.  The same layer, since row scaling commutes
with the down projection; the rounding differs (w meets h before the GEMM,
not its output after).

Layout.  Slot s = t*k + j is token t's j-th selected expert.  `dest[s]` is
the slot's row in the expert-sorted layout (rows of one expert contiguous,
ordered by s: the stable sort by expert) and `offs[e]` the inclusive
cumulative row count per expert, the format F.grouped_mm takes.

The router weights stay f32 until the combine, which rounds once; HF's
Qwen3MoE rounds them to the activation dtype first.

Router auxiliary losses (moe_router(..., aux=True), moe_router_aux.hip): the
load-balancing loss of Switch / HF, aux = E * sum_e (c[e] / T) * P[e] with
c[e] the slots routed to expert e and P[e] the mean FULL-softmax probability
of e (in both norm_topk_prob modes), and the router z-loss of ST-MoE,
z = mean_t logsumexp(x[t])^2, come out of the router kernels with their
gradients.  Two conventions differ from HF's Qwen3MoE: HF pools the tokens
of all layers before forming c and P, while here every layer forms its own
over the T tokens it sees and the model averages the layers' losses (the
Switch / Megatron convention); and under data parallelism the statistics are
per rank and per micro-batch, with no collective.

Not done: expert parallelism, capacity limits / token dropping, shared
experts."""
import warnings

import torch
import torch.nn.functional as F

from .._ext import ext, use_hip
from .swiglu import silu_mul

ROUTER_EXPERTS = (8, 16, 32, 64, 128)
MAX_TOP_K = 8


# --------------------------------------------------------------------------
# router
# --------------------------------------------------------------------------
class _RouterFn(torch.autograd.Function):
    """Saves the logits and the selection; the probabilities are recomputed
    in the backward."""

    @staticmethod
    def forward(ctx, logits, k, norm):
        idx, w = ext().moe_router_fwd(logits, k, norm)
        ctx.save_for_backward(logits, idx)
        ctx.norm = norm
        ctx.mark_non_differentiable(idx)
        return idx, w

    @staticmethod
    def backward(ctx, _didx, dw):
        logits, idx = ctx.saved_tensors
        return ext().moe_router_bwd(logits, idx, dw.contiguous(),
                                    ctx.norm), None, None


class _RouterAuxFn(torch.autograd.Function):
    """_RouterFn with the two auxiliary losses as further outputs.  Saves
    the expert counts as well; a missing upstream gradient counts as zero
    and the scalars' gradients reach the kernel as device tensors."""

    @staticmethod
    def forward(ctx, logits, k, norm):
        idx, w, counts, aux, z = ext().moe_router_aux_fwd(logits, k, norm)
        ctx.save_for_backward(logits, idx, counts)
        ctx.norm = norm
        ctx.mark_non_differentiable(idx)
        return idx, w, aux, z

    @staticmethod
    def backward(ctx, _didx, dw, daux, dz):
        logits, idx, counts = ctx.saved_tensors
        dw = torch.zeros(idx.shape, dtype=torch.float32,
                         device=idx.device) if dw is None else dw.contiguous()
        daux, dz = (logits.new_zeros((), dtype=torch.float32) if g is None
                    else g.float().contiguous() for g in (daux, dz))
        return ext().moe_router_aux_bwd(logits, idx, dw, counts, daux, dz,
                                        ctx.norm), None, None


def moe_router_eager(logits, k, norm_topk_prob=True, aux=False):
    """The router in torch ops, f32, differentiable (any device); with `aux`
    the two auxiliary losses of moe_router as well."""
    x = logits.float()
    # stable descending sort: a tie goes to the lower expert index
    idx = torch.sort(-x.detach(), dim=-1, stable=True).indices[:, :k]
    if norm_topk_prob:
        w = torch.softmax(x.gather(1, idx), dim=-1)
    else:
        w = torch.softmax(x, dim=-1).gather(1, idx)
    if not aux:
        return idx.to(torch.int32), w
    T, E = x.shape
    lse = torch.logsumexp(x, dim=-1)
    counts = torch.bincount(idx.reshape(-1), minlength=E).to(x.dtype)
    p_mean = torch.exp(x - lse.unsqueeze(1)).mean(0)
    return (idx.to(torch.int32), w, E * (counts / T * p_mean).sum(),
            lse.square().mean())


def moe_router(logits, k, norm_topk_prob=True, aux=False):
    """Top-k routing over router logits [T, E] (bf16 on the GPU).

    Returns (topk_idx int32 [T, k], topk_w f32 [T, k]).  The selection runs
    on the logits widened to f32, in descending order, a tie going to the
    lower expert index (the first k of a stable descending sort).  With
    norm_topk_prob (Qwen3-MoE) the weights are the softmax over the k
    selected logits, otherwise the full softmax's values at the selection.
    All arithmetic is f32 and the weights are returned in f32.

    With `aux` it returns (topk_idx, topk_w, aux, z): the load-balancing
    loss and the router z-loss of these T tokens (the module docstring has
    the definitions) as 0-dim f32, differentiable; topk_idx and topk_w are
    the same bits.  The losses always use the full softmax.

    On the GPU E must be one of ROUTER_EXPERTS and 1 <= k <= min(8, E)."""
    T, E = logits.shape
    if not 1 <= k <= E:
        raise ValueError(f"moe_router: k must be in [1, {E}], got {k}")
    if aux and T < 1:
        raise ValueError("moe_router: the auxiliary losses need a token")
    if use_hip(logits):
        if E not in ROUTER_EXPERTS or k > MAX_TOP_K:
            raise ValueError(
                f"moe_router: the GPU kernel takes E in {ROUTER_EXPERTS} and "
                f"k <= {MAX_TOP_K}, got E={E}, k={k}")
        fn = _RouterAuxFn if aux else _RouterFn
        return fn.apply(logits.contiguous(), int(k), bool(norm_topk_prob))
    return moe_router_eager(logits, k, norm_topk_prob, aux)


# --------------------------------------------------------------------------
# expert-sorted layout
# --------------------------------------------------------------------------
def moe_dispatch_index_eager(topk_idx, num_experts):
    """(dest, offs) by a stable sort (any device)."""
    flat = topk_idx.reshape(-1).long()
    order = torch.sort(flat, stable=True).indices
    dest = torch.empty_like(order)
    dest[order] = torch.arange(flat.numel(), device=flat.device)
    offs = torch.bincount(flat, minlength=num_experts).cumsum(0)
    return dest.to(torch.int32), offs.to(torch.int32)


def moe_dispatch_index(topk_idx, num_experts):
    """Expert-sorted layout of the slots of topk_idx [T, k] (values in
    [0, num_experts)): (dest int32 [T*k], offs int32 [num_experts]).

    dest[t*k + j] is the slot's row; rows of one expert are contiguous and
    ordered by slot.  offs is the inclusive cumulative row count per expert.
    Built on the device without a host sync or atomics; bitwise
    reproducible.  Carries no gradient."""
    if use_hip(topk_idx):
        dest, offs = ext().moe_dispatch_index(
            topk_idx.to(torch.int32).contiguous(), int(num_experts))
        return dest, offs
    return moe_dispatch_index_eager(topk_idx, num_experts)


class _ScatterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dest, k):
        ctx.save_for_backward(dest)
        ctx.k = k
        return ext().moe_scatter(x, dest)

    @staticmethod
    def backward(ctx, dxp):
        (dest,) = ctx.saved_tensors
        # dx[t] = sum_j dxp[dest[t*k + j]]: the combine with weights of one
        return ext().moe_combine(dxp.contiguous(), dest, None, ctx.k), \
            None, None


def _rows_of(dest, k):
    """token of every row of the sorted layout (the inverse of dest, / k)"""
    inv = torch.empty_like(dest, dtype=torch.long)
    inv[dest.long()] = torch.arange(dest.numel(), device=dest.device)
    return inv, torch.div(inv, k, rounding_mode="floor")


def moe_scatter_eager(x, dest, k):
    return x.index_select(0, _rows_of(dest, k)[1])


def moe_scatter(x, dest, k):
    """xp [T*k, H] with xp[dest[t*k + j]] = x[t] for every slot: the tokens
    in expert-sorted order, each row a bit-exact copy.  x is [T, H] (bf16
    with H % 8 == 0 on the GPU); dest must be a permutation of [0, T*k)."""
    if dest.numel() != x.shape[0] * k:
        raise ValueError("moe_scatter: dest must hold k slots per row of x")
    if use_hip(x):
        return _ScatterFn.apply(x.contiguous(), dest, int(k))
    return moe_scatter_eager(x, dest, k)


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, yp, dest, w):
        ctx.save_for_backward(yp, dest, w)
        return ext().moe_combine(yp, dest, w, w.shape[1])

    @staticmethod
    def backward(ctx, dy):
        yp, dest, w = ctx.saved_tensors
        # one pass: dyp[dest[s]] = w[s] * dy[t] and dw[s] = <dy[t], yp[..]>
        dyp, dw = ext().moe_combine_bwd(dy.contiguous(), dest, w, yp)
        return dyp, None, dw


def moe_combine_eager(yp, dest, w):
    """The classic chain: weigh the sorted rows, index_add_ them into an f32
    accumulator per token, round once."""
    T, k = w.shape
    inv, tok = _rows_of(dest, k)
    rows = yp.float() * w.reshape(-1)[inv].unsqueeze(1)
    y = torch.zeros(T, yp.shape[1], dtype=torch.float32, device=yp.device)
    return y.index_add(0, tok, rows).to(yp.dtype)


def moe_combine(yp, dest, w):
    """y [T, H] = sum_j w[t, j] * yp[dest[t*k + j]]: the experts' outputs
    back in token order, accumulated in f32 in fixed j order and rounded
    once.  yp is [T*k, H], w f32 [T, k]."""
    if w.dim() != 2 or dest.numel() != w.numel() \
            or yp.shape[0] != dest.numel():
        raise ValueError("moe_combine: yp [T*k, H], dest [T*k], w [T, k]")
    if use_hip(yp):
        return _CombineFn.apply(yp.contiguous(), dest,
                                w.float().contiguous())
    return moe_combine_eager(yp, dest, w)


# --------------------------------------------------------------------------
# expert GEMMs and the composed layer
# --------------------------------------------------------------------------
# "grouped", "loop", "hip", "hip-gather" or "hip-fused" (set by moe_mlp's fused
# chain): which path the last expert GEMM took
# (reporting only; the torch decision is kept per device type in
# _grouped_mm_works)
last_expert_mm_path = None
_grouped_mm_works = {}  # device type -> bool, decided by the first call
EXPERT_GEMM_IMPLS = ("torch", "hip", "hip-gather", "hip-fused")
MOE_GEMM_MAX_EXPERTS = 128


def moe_row_src(dest, k):
    """row_src int32 [T*k]: the token of every row of the expert-sorted
    layout, row_src[dest[t*k + j]] = t.  What the gather-fused expert GEMMs
    read x through instead of a scattered copy."""
    if use_hip(dest):
        return ext().moe_row_src(dest.contiguous(), int(k))
    return _rows_of(dest, k)[1].to(torch.int32)


def moe_row_w(dest, topk_w):
    """w_row f32 [T*k]: the router weight of every row of the expert-sorted
    layout, w_row[dest[t*k + j]] = topk_w[t, j].  Carries no gradient: the
    fused chain forms topk_w's gradient itself."""
    if use_hip(dest):
        return ext().moe_row_w(dest.contiguous(),
                               topk_w.detach().float().contiguous())
    out = torch.empty(dest.numel(), dtype=torch.float32, device=dest.device)
    out[dest.long()] = topk_w.detach().float().reshape(-1)
    return out


def _expert_mm_loop(a, weight, offs):
    lo, parts = 0, []
    for e, hi in enumerate(offs.tolist()):  # one host read
        parts.append(F.linear(a[lo:hi], weight[e]))
        lo = hi
    return torch.cat(parts)


class _ExpertMMFn(torch.autograd.Function):
    """The three grouped GEMMs of moe_gemm.hip: y = a . w[e]^T forward,
    da = dy . w[e] and dw[e] = dy[rows e]^T . a[rows e] backward.  offs stays
    on the device throughout."""

    @staticmethod
    def forward(ctx, a, weight, offs):
        ctx.save_for_backward(a, weight, offs)
        return ext().moe_gemm_rows(a, weight, offs, False)

    @staticmethod
    def backward(ctx, dy):
        a, weight, offs = ctx.saved_tensors
        dy = dy.contiguous()
        da = ext().moe_gemm_rows(dy, weight, offs, True) \
            if ctx.needs_input_grad[0] else None
        dw = ext().moe_gemm_dw(dy, a, offs) \
            if ctx.needs_input_grad[1] else None
        return da, dw, None


class _ExpertMMGatherFn(torch.autograd.Function):
    """_ExpertMMFn on the unsorted tokens x [T, K] (moe_gemm_gather.hip):
    y[r] = x[row_src[r]] . w[e]^T.  Saves x, which the router projection
    keeps alive anyway, and never an [N, K] tensor; row_src is 4 bytes a row
    and one small launch, so the backward rebuilds it from dest rather than
    keep it.  dx is the k-way sum of the sorted dxp (the scatter's backward),
    dw reads x through row_src again."""

    @staticmethod
    def forward(ctx, x, weight, offs, dest, row_src):
        ctx.save_for_backward(x, weight, offs, dest)
        return ext().moe_gemm_rows_gather(x, row_src, weight, offs)

    @staticmethod
    def backward(ctx, dy):
        x, weight, offs, dest = ctx.saved_tensors
        dy = dy.contiguous()
        k = dest.numel() // x.shape[0]
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dxp = ext().moe_gemm_rows(dy, weight, offs, True)
            dx = ext().moe_combine(dxp, dest, None, k)
        if ctx.needs_input_grad[1]:
            dw = ext().moe_gemm_dw_gather(dy, x, ext().moe_row_src(dest, k),
                                          offs)
        return dx, dw, None, None, None


class _GateUpSwigluFn(_ExpertMMGatherFn):
    """_ExpertMMGatherFn for gate_up with the weighted SwiGLU in the epilogue
    (moe_gemm_swiglu.hip): (gu, h') with gu[r] = x[row_src[r]] . gate_up[e]^T,
    the bits of that function, and h' = bf16(w_r * silu(g_r) * u_r).  h' is
    not differentiable here: _DownSwigluFn, the one place it goes, hands back
    the gradient of gu, which the inherited backward takes to dx and the
    weight gradient.  topk_w's gradient comes from there as well."""

    @staticmethod
    def forward(ctx, x, gate_up, topk_w, offs, dest):
        k = topk_w.shape[1]
        gu, hw = ext().moe_gemm_gu_swiglu(
            x, ext().moe_row_src(dest, k), ext().moe_row_w(dest, topk_w),
            gate_up, offs)
        ctx.save_for_backward(x, gate_up, offs, dest)
        ctx.mark_non_differentiable(hw)
        return gu, hw

    @staticmethod
    def backward(ctx, dgu, _dhw):
        return _ExpertMMGatherFn.backward(ctx, dgu)


class _DownSwigluFn(torch.autograd.Function):
    """yp = h' . down[e]^T as a function of gu, w and down, h' being
    w * silu(g) * u: the rows come out sorted and already weighted.  Saves gu
    and h', never yp and never dh: the backward's dA kernel turns
    dyp . down[e] into dgu and topk_w's gradient in its epilogue.  w_row is
    one small launch and is rebuilt rather than kept.  A function of its own,
    so that dyp is released before the gate_up backward allocates."""

    @staticmethod
    def forward(ctx, gu, hw, down, topk_w, offs, dest):
        ctx.save_for_backward(gu, hw, down, topk_w, offs, dest)
        return ext().moe_gemm_rows(hw, down, offs, False)

    @staticmethod
    def backward(ctx, dyp):
        gu, hw, down, topk_w, offs, dest = ctx.saved_tensors
        dyp = dyp.contiguous()
        dgu, dw = ext().moe_gemm_da_swiglu(
            dyp, down, gu, ext().moe_row_w(dest, topk_w), offs, dest)
        ddown = ext().moe_gemm_dw(dyp, hw, offs) \
            if ctx.needs_input_grad[2] else None
        return dgu, None, ddown, dw.view_as(topk_w), None, None


class _SumFn(torch.autograd.Function):
    """The unweighted combine, y[t] = sum_j yp[dest[t*k + j]]: _ScatterFn's
    mirror.  Saves dest alone."""

    @staticmethod
    def forward(ctx, yp, dest, k):
        ctx.save_for_backward(dest)
        return ext().moe_combine(yp, dest, None, k)

    @staticmethod
    def backward(ctx, dy):
        (dest,) = ctx.saved_tensors
        return ext().moe_scatter(dy.contiguous(), dest), None, None


def moe_gemm_supported(a, weight):
    """What moe_gemm.hip serves: bf16 on the GPU, E <= 128, M and K
    multiples of 64 (any N, any rows per expert)."""
    E, M, K = weight.shape
    return use_hip(a) and a.dtype == weight.dtype == torch.bfloat16 \
        and weight.device == a.device and 1 <= E <= MOE_GEMM_MAX_EXPERTS \
        and M >= 64 and M % 64 == 0 and K >= 64 and K % 64 == 0


def expert_mm(a, weight, offs, impl="torch", row_src=None, dest=None):
    """Rows [offs[e-1], offs[e]) of a [N, K] times weight[e].T, for weight
    [E, M, K]: the one helper both expert GEMMs go through.  torch's grouped
    GEMM takes the device-side offsets, so nothing waits on the host.

    impl="hip" takes the hand-written grouped GEMMs of moe_gemm.hip, forward
    and backward, where moe_gemm_supported holds (no host read of offs, no
    dependence on torch's grouped GEMM); on a CPU tensor or another shape or
    dtype it is the torch path below, unchanged.

    With `row_src` (moe_row_src) and the `dest` it was built from, a is the
    unsorted [T, K] token tensor and row r of the product is
    a[row_src[r]] . weight[e].T.  impl="hip-gather" then runs the kernels of
    moe_gemm_gather.hip, which read a through row_src in the forward and in
    the weight gradient, so no [N, K] copy is made or saved; the results are
    the bits impl="hip" gives on moe_scatter(a, dest, k).  Where
    moe_gemm_supported fails, or under another impl, the rows are scattered
    first and the call goes on as without row_src.  Without row_src
    "hip-gather" is "hip".  "hip-fused" is "hip-gather" here: its fusion
    spans both GEMMs and lives in moe_mlp.

    Where this build of torch cannot run the grouped GEMM on a's kind of
    device, the helper warns once and from then on loops over the experts'
    row slices on that kind of device, at the cost of one host read of offs
    per call.  Only the first call on a device type decides, and only a
    refusal decides: the arguments are checked here first, so a caller's
    shape error is a ValueError, and running out of memory is re-raised."""
    global last_expert_mm_path
    if impl not in EXPERT_GEMM_IMPLS:
        raise ValueError(
            f"expert_mm: impl must be one of {EXPERT_GEMM_IMPLS}, got {impl!r}")
    if a.dim() != 2 or weight.dim() != 3 or a.shape[1] != weight.shape[2] \
            or offs.shape != (weight.shape[0],) or offs.dtype != torch.int32:
        raise ValueError(
            f"expert_mm: a [N, K], weight [E, M, K], offs int32 [E]; got "
            f"{tuple(a.shape)}, {tuple(weight.shape)}, {tuple(offs.shape)} "
            f"{offs.dtype}")
    if row_src is not None:
        if dest is None or a.shape[0] < 1 or row_src.shape != dest.shape \
                or dest.dim() != 1 or dest.numel() % a.shape[0] != 0:
            raise ValueError(
                "expert_mm: with row_src, a is [T, K] with T >= 1 and "
                "row_src and dest are both [T*k]")
        if impl in ("hip-gather", "hip-fused") \
                and moe_gemm_supported(a, weight):
            last_expert_mm_path = "hip-gather"
            return _ExpertMMGatherFn.apply(a.contiguous(),
                                           weight.contiguous(), offs, dest,
                                           row_src)
        a = moe_scatter(a, dest, dest.numel() // a.shape[0])
    if impl != "torch" and moe_gemm_supported(a, weight):
        last_expert_mm_path = "hip"
        return _ExpertMMFn.apply(a.contiguous(), weight.contiguous(), offs)
    kind = a.device.type
    if _grouped_mm_works.get(kind, True):
        try:
            out = F.grouped_mm(a, weight.transpose(-2, -1), offs=offs)
            _grouped_mm_works[kind] = True
            last_expert_mm_path = "grouped"
            return out
        except torch.OutOfMemoryError:
            raise
        except (RuntimeError, NotImplementedError) as e:
            if _grouped_mm_works.get(kind):
                raise  # it has worked here before: an error of this call
            _grouped_mm_works[kind] = False
            warnings.warn(
                f"F.grouped_mm is not usable on {kind} in this torch build "
                f"({e}); the expert GEMMs fall back to a per-expert loop "
                "with one host sync per call", RuntimeWarning, stacklevel=2)
    last_expert_mm_path = "loop"
    return _expert_mm_loop(a, weight, offs)


def _fused_supported(x, gate_up, down):
    """What moe_gemm_swiglu.hip serves: moe_gemm_supported for both GEMMs,
    at least one token, and I a multiple of 64."""
    return x.shape[0] > 0 and gate_up.shape[1] % 128 == 0 \
        and moe_gemm_supported(x, gate_up) \
        and down.shape == (gate_up.shape[0], x.shape[1],
                           gate_up.shape[1] // 2) \
        and down.dtype == x.dtype and down.device == x.device


def _mlp_chain(x, router_weight, gate_up, down, k, norm, aux, router, index,
               scatter, combine, expert_gemm="torch"):
    global last_expert_mm_path
    E = gate_up.shape[0]
    logits = F.linear(x, router_weight)
    # without aux the router is called exactly as before the option existed
    idx, w, *losses = router(logits, k, norm, True) if aux \
        else router(logits, k, norm)
    dest, offs = index(idx, E)
    if expert_gemm == "hip-fused":
        if _fused_supported(x, gate_up, down):
            last_expert_mm_path = "hip-fused"
            w = w.float().contiguous()
            gu, hw = _GateUpSwigluFn.apply(x.contiguous(),
                                           gate_up.contiguous(), w, offs, dest)
            y = _SumFn.apply(_DownSwigluFn.apply(gu, hw, down.contiguous(), w,
                                                 offs, dest), dest, k)
            return (y, *losses) if aux else y
        expert_gemm = "hip-gather"  # the same layer, rounded elsewhere
    if expert_gemm == "hip-gather" and x.shape[0] > 0 \
            and moe_gemm_supported(x, gate_up):
        # gate_up reads x through the row index; h is born sorted, so the
        # down GEMM below is the plain "hip" one
        gu = expert_mm(x, gate_up, offs, expert_gemm,
                       row_src=moe_row_src(dest, k), dest=dest)
    else:
        gu = expert_mm(scatter(x, dest, k), gate_up, offs, expert_gemm)
    h = silu_mul(gu)
    y = combine(expert_mm(h, down, offs, expert_gemm), dest, w)
    return (y, *losses) if aux else y


def moe_mlp_eager(x, router_weight, gate_up, down, k, norm_topk_prob=True,
                  aux=False):
    """moe_mlp as the torch-op chain (stable sort, index_select, the same
    GEMM helper, index_add_ in f32), on any device: the CPU path, and what
    the fused path is compared and benchmarked against."""
    return _mlp_chain(x, router_weight, gate_up, down, k, norm_topk_prob, aux,
                      moe_router_eager, moe_dispatch_index_eager,
                      moe_scatter_eager, moe_combine_eager)


def moe_mlp(x, router_weight, gate_up, down, k, norm_topk_prob=True,
            aux=False, expert_gemm="torch"):
    """A mixture-of-experts SwiGLU feed-forward over tokens x [T, H].

    router_weight [E, H]; gate_up [E, 2I, H] (gate | up packed, so silu_mul
    serves the activation on the sorted rows); down [E, H, I].  Every token
    goes through its k routed experts and the outputs are summed with the
    router's weights.  With `aux` it returns (y, aux, z), the router's two
    auxiliary losses over these tokens (moe_router).  `expert_gemm` is
    expert_mm's `impl` for both expert GEMMs.  "hip-gather" is "hip" without
    the scattered copy of x: the gate_up GEMM and its weight gradient read x
    through moe_row_src's index (moe_gemm_gather.hip), which keeps T*k*H
    bf16 less alive until the backward; outputs and gradients are the same
    bits.  "hip-fused" is "hip-gather" with the weighted SwiGLU in the GEMMs'
    epilogues (moe_gemm_swiglu.hip, I % 64 == 0): the router weight scales h
    before the down GEMM, the combine sums unweighted and the sorted down
    output [T*k, H] is not kept for the backward.  The same mathematics with
    another rounding; on CPU tensors or unsupported shapes it is
    "hip-gather" with that value's own fallbacks."""
    if expert_gemm not in EXPERT_GEMM_IMPLS:
        raise ValueError(f"moe_mlp: expert_gemm must be one of "
                         f"{EXPERT_GEMM_IMPLS}, got {expert_gemm!r}")
    if use_hip(x):
        return _mlp_chain(x, router_weight, gate_up, down, k, norm_topk_prob,
                          aux, moe_router, moe_dispatch_index, moe_scatter,
                          moe_combine, expert_gemm)
    return moe_mlp_eager(x, router_weight, gate_up, down, k, norm_topk_prob,
                         aux)
