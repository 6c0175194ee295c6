"""fp8_quant.hip through ops.fp8_quantize: exact checks, no tolerance.

The reference is eager torch on the CPU, fed the kernel's own input:

    amax      = x.abs().max()
    scale     = 448 / clamp(amax, 1e-12)        (fp32, one IEEE division)
    inv_scale = clamp(amax, 1e-12) / 448        (fp32, one IEEE division)
    q         = (x.float() * scale).clamp(-448, 448).to(float8_e4m3fn)

which rounds to nearest-even and keeps -0.  Both quotients are taken between
two fp32 tensors: Python's `448.0 / tensor` is torch's reciprocal followed by
a multiply, two roundings, and is not the division the scales are defined by
(it differs in the last bit for about a third of all amax values).  Scales
are compared bit for bit, q and qt byte for byte.  Each (shape, recipe) case
is computed once and shared by the tests below."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_training_guide_amd._ext import ext
from distributed_training_guide_amd.ops import fp8_quantize

FP8 = torch.float8_e4m3fn

# single tile, exact tile, a partial tile in each direction (64x64 tiles),
# many tiles
SHAPES = [(16, 16), (64, 64), (48, 80), (208, 80), (80, 208), (256, 4096)]
RECIPES = ["randn_1e-3", "randn_1", "randn_1e3", "pinned_first",
           "pinned_last", "pinned_partial", "zeros"]

# bf16 inputs and what they become at scale == 1.0 (ties go to the even
# e4m3 mantissa; 447 is already 448 in bf16; 2^-9 is e4m3's smallest
# subnormal, so 2^-10 is a tie with 0)
PINNED = [17.0, 19.0, 447.0, 2.0 ** -10, 3 * 2.0 ** -10, 0.001, -0.0]
PINNED_Q = [16.0, 20.0, 448.0, 0.0, 2.0 ** -8, 2.0 ** -9, -0.0]


def _amax_index(recipe, R, C):
    return {"pinned_first": (0, 0), "pinned_last": (R - 1, C - 1),
            # three rows and five columns from the end: inside the last tile,
            # which hangs over the edge in every shape that has one
            "pinned_partial": (R - 3, C - 5)}[recipe]


def _pinned_slots(R, C):
    """(row, first column) of the two runs of PINNED: the tensor's start
    (after the possible amax element) and its last row."""
    return [(0, 1), (R - 1, C - 15)]


def _input(shape, recipe):
    R, C = shape
    g = torch.Generator(device="cpu").manual_seed(R * 10007 + C)
    if recipe == "zeros":
        return torch.zeros(R, C, dtype=torch.bfloat16)
    if recipe.startswith("randn_"):
        return (torch.randn(R, C, generator=g)
                * float(recipe.split("_")[1])).bfloat16()
    # pinned: everything below 448, exactly one element at +-448
    x = (torch.randn(R, C, generator=g) * 30.0).clamp(-400.0, 400.0)
    for r, c in _pinned_slots(R, C):
        x[r, c:c + len(PINNED)] = torch.tensor(PINNED)
    x[_amax_index(recipe, R, C)] = -448.0 if recipe == "pinned_last" \
        else 448.0
    return x.bfloat16()


def _bytes(t):
    return t.view(torch.uint8)


@functools.lru_cache(maxsize=None)
def _case(shape, recipe):
    x_cpu = _input(shape, recipe)
    amax = x_cpu.abs().max().float()
    e4m3_max = torch.tensor(448.0, dtype=torch.float32)
    scale = torch.div(e4m3_max, amax.clamp(min=1e-12))
    inv_scale = torch.div(amax.clamp(min=1e-12), e4m3_max)
    q_ref = (x_cpu.float() * scale).clamp(-448.0, 448.0).to(FP8)
    x = x_cpu.cuda()
    q, qt, s, inv_s = fp8_quantize(x, rowwise=True, transposed=True)
    torch.cuda.synchronize()
    return dict(x=x, x_cpu=x_cpu, scale_ref=scale, inv_scale_ref=inv_scale,
                q_ref=q_ref, q=q, qt=qt, scale=s, inv_scale=inv_s)


CASES = [(s, r) for s in SHAPES for r in RECIPES]
case_ids = [f"{s[0]}x{s[1]}-{r}" for s, r in CASES]
cases = pytest.mark.parametrize("shape,recipe", CASES, ids=case_ids)


def _same_bits_f32(a, b):
    return torch.equal(a.detach().cpu().reshape(1).view(torch.int32),
                       b.detach().cpu().reshape(1).view(torch.int32))


@cases
def test_scales_bit_equal(shape, recipe):
    c = _case(shape, recipe)
    assert c["scale"].dtype == torch.float32 and c["scale"].is_cuda
    assert c["inv_scale"].dtype == torch.float32 and c["inv_scale"].is_cuda
    print("scale", c["scale"].item(), c["scale_ref"].item(),
          "inv_scale", c["inv_scale"].item(), c["inv_scale_ref"].item())
    assert _same_bits_f32(c["scale"], c["scale_ref"])
    assert _same_bits_f32(c["inv_scale"], c["inv_scale_ref"])
    assert torch.isfinite(c["scale"]).item()
    assert torch.isfinite(c["inv_scale"]).item()
    if recipe.startswith("pinned"):
        assert c["scale"].item() == 1.0


@cases
def test_q_bytes_equal_torch_cast(shape, recipe):
    c = _case(shape, recipe)
    q = c["q"]
    assert q.dtype == FP8 and q.shape == c["x"].shape and q.is_contiguous()
    got, ref = _bytes(q).cpu(), _bytes(c["q_ref"])
    bad = (got != ref).nonzero()
    if len(bad):
        r, col = (int(i) for i in bad[0])
        raise AssertionError(
            f"{len(bad)} of {got.numel()} bytes differ; first at ({r}, "
            f"{col}): x={c['x_cpu'][r, col].item()!r} scale="
            f"{c['scale_ref'].item()!r} got 0x{int(got[r, col]):02x} "
            f"reference 0x{int(ref[r, col]):02x}")
    if recipe == "zeros":
        assert not got.any()


@cases
def test_qt_is_q_transposed(shape, recipe):
    c = _case(shape, recipe)
    R, C = shape
    assert c["qt"].dtype == FP8 and c["qt"].shape == (C, R)
    assert c["qt"].is_contiguous()
    assert torch.equal(_bytes(c["qt"]), _bytes(c["q"]).t())


@cases
def test_single_output_calls_match_both(shape, recipe):
    c = _case(shape, recipe)
    q1, none_t, s1, i1 = fp8_quantize(c["x"], rowwise=True, transposed=False)
    none_q, qt2, s2, i2 = fp8_quantize(c["x"], rowwise=False,
                                       transposed=True)
    assert none_t is None and none_q is None
    assert torch.equal(_bytes(q1), _bytes(c["q"]))
    assert torch.equal(_bytes(qt2), _bytes(c["qt"]))
    for s, i in ((s1, i1), (s2, i2)):
        assert _same_bits_f32(s, c["scale"])
        assert _same_bits_f32(i, c["inv_scale"])


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
def test_supplied_scale_is_used(shape):
    c = _case(shape, "randn_1")
    # 200 overflows randn into the clamp; 0.37 is no power of two
    for value in (200.0, 0.37):
        scale = torch.tensor([value], dtype=torch.float32)
        ref = (c["x_cpu"].float() * scale).clamp(-448.0, 448.0).to(FP8)
        q, qt, s, inv_s = fp8_quantize(c["x"], rowwise=True, transposed=True,
                                       scale=scale.cuda())
        assert inv_s is None and _same_bits_f32(s, scale)
        assert torch.equal(_bytes(q).cpu(), _bytes(ref))
        assert torch.equal(_bytes(qt), _bytes(q).t())
        _, qt_only, _, _ = fp8_quantize(c["x"], rowwise=False,
                                        transposed=True, scale=scale.cuda())
        assert torch.equal(_bytes(qt_only), _bytes(qt))


@pytest.mark.parametrize("recipe", ["pinned_first", "pinned_last",
                                    "pinned_partial"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
def test_pinned_values(shape, recipe):
    """Ties, the subnormal range and -0 at scale == 1.0, as the values
    themselves and not only as agreement with the reference."""
    c = _case(shape, recipe)
    R, C = shape
    want = torch.tensor(PINNED_Q)
    want_bytes = _bytes(want.to(FP8))
    assert int(want_bytes[-1]) == 0x80 and int(want_bytes[3]) == 0x00
    q = c["q"].cpu()
    for r, col in _pinned_slots(R, C):
        got = q[r, col:col + len(PINNED)]
        assert torch.equal(_bytes(got), want_bytes), (r, col, got.float())
    ar, ac = _amax_index(recipe, R, C)
    assert abs(q[ar, ac].float().item()) == 448.0
    assert torch.equal(_bytes(c["qt"]).cpu()[ac, ar], _bytes(q)[ar, ac])


def test_binding_rejects_malformed_arguments():
    e = ext()
    x = torch.randn(32, 48, device="cuda").bfloat16()
    scale = torch.ones(1, device="cuda")
    e.fp8_amax_scale(x)
    e.fp8_cast_transpose(x, scale, True, True)
    bad = [
        (x.float(), "must be bf16"),
        (x.t(), "must be contiguous"),
        (x[:, ::2], "must be contiguous"),
        (x.cpu(), "must be on the GPU"),
        (x[:24].contiguous(), "multiples of 16"),
        (x[:, :40].contiguous(), "multiples of 16"),
        (x.reshape(2, 16, 48), "2-D"),
    ]
    for arg, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            e.fp8_amax_scale(arg)
        with pytest.raises(RuntimeError, match=msg):
            e.fp8_cast_transpose(arg, scale, True, True)
    with pytest.raises(RuntimeError, match="scale must be on x's device"):
        e.fp8_cast_transpose(x, scale.cpu(), True, True)
    with pytest.raises(RuntimeError, match="single f32 value"):
        e.fp8_cast_transpose(x, torch.ones(2, device="cuda"), True, True)
    with pytest.raises(RuntimeError, match="single f32 value"):
        e.fp8_cast_transpose(x, scale.double(), True, True)
    with pytest.raises(RuntimeError, match="at least one output"):
        e.fp8_cast_transpose(x, scale, False, False)
    # the public op checks the same before it reaches the binding
    with pytest.raises(ValueError, match="multiples of 16"):
        fp8_quantize(x[:24].contiguous())
    with pytest.raises(TypeError, match="bf16"):
        fp8_quantize(x.float())
