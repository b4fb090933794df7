"""GPU (MI355X): the backward of transform / inverse_transform -- the transposed bank of ac_mdct_plan_adjoint run by the
synthesis / analysis kernels -- against torch.autograd on the float64 restatement of the filter bank
(tests/mdct_torch_reference.py), over the whole gradient tensor, on every tier the adjoint plan runs: the wave-level
kernels (tier 3, one and several frames per wave, the four-coefficient FOLD4 form), the compile-time LDS-FFT instances
(tier 2, the channel-team forms for C >= 3 included), the tier's run-time forms (tier 1) and the O(N^2) kernels (tier 0,
which also serve the forced-generic runs), in float32, float64, bfloat16 and float16.  Every case pins the tier of the
plan and of the adjoint plan, so a silent change of route fails instead of passing the numerics.

Bars (peak = max|g - g_ref| / max|g_ref| and rel-L2 = ||g - g_ref|| / ||g_ref||, over the whole tensor).  The worst
values measured on the MI355X over every case of this module:
  * tier3 (float32, wave-level kernels):         peak 5.3e-7, rel-L2 1.4e-7
  * tier2 (float32, LDS-FFT instances):          peak 2.1e-7, rel-L2 1.4e-7
  * tier1 (float32, LDS-FFT run-time forms):     peak 1.8e-7, rel-L2 1.3e-7
  * tier0 (float32, O(N^2) kernels):             peak 5.1e-7, rel-L2 9.5e-8
  * float64 (O(N^2) kernels in double):          peak 5.7e-15, rel-L2 2.2e-15
  * bfloat16 (float32 inside, rounded once):     peak 3.0e-3, rel-L2 1.7e-3
  * float16 (float32 inside, rounded once):      peak 4.4e-4, rel-L2 2.2e-4
Each bar is about 4x the worst value of its path.  Every bfloat16 / float16 gradient is also within half an ulp of its
storage type at every element plus the float32 tier's peak bar times the peak: what one rounding of a float32 result
allows, and what a gradient rounded twice (stored, then scaled by a 4N that is not a power of two) does not meet: the
backward that stored 4N T^T g and S^T g / 4N in the 2-byte type failed it at N = 960 and 34, and gave inf in x.grad and
subnormal garbage in X.grad for the float16 range cases.  Every
parametrised case shows its bar is not vacuous: it rejects the reference with the first block's gradient zeroed (the
x_-1 = 0 edge), the reference with one fold position's coefficients negated, and, for the rectangular window, the
orthogonal-fold shortcut T^T g = inverse_transform(g) / 4N.
"""

import numpy as np
import pytest
import torch

import mdct_torch_reference as ref

import audiocodec_amd
from audiocodec_amd import _lib

pytestmark = pytest.mark.gpu

# (peak, rel-L2) per path; see the module docstring for the measured worst values
BARS = {"tier3": (2.2e-6, 6e-7), "tier2": (8e-7, 6e-7), "tier1": (7e-7, 5e-7), "tier0": (2e-6, 4e-7),
        "float64": (2.3e-14, 9e-15), "bfloat16": (1.2e-2, 7e-3), "float16": (1.8e-3, 9e-4)}
WORST = {}
F16_TINY = 2.0 ** -14          # float16's smallest normal


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X (run with -m gpu on the GPU box)"
    assert _lib.load().ac_set_force_generic(0) == 0, "AC_TESTING=1 not in effect"
    yield
    _lib.load().ac_set_force_generic(0)
    if WORST:
        print("\nworst gradient errors (peak, rel-L2) per path:")
        for k in sorted(WORST):
            print("  %-9s %.2e  %.2e" % (k, *WORST[k]))


def _errs(g, r):
    g, r = g.detach().double().cpu(), r.detach().double().cpu()
    d = g - r
    return float(d.abs().max() / r.abs().max()), float(torch.linalg.vector_norm(d) / torch.linalg.vector_norm(r))


def _within(g, r, path):
    peak, l2 = _errs(g, r)
    return peak <= BARS[path][0] and l2 <= BARS[path][1]


def _half_ulp(v, dt):
    """Half the spacing of ``dt`` (float16 / bfloat16) at |v|, subnormals included, as float64."""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dt]
    _, e = torch.frexp(v.abs())                         # |v| = m 2^e, m in [0.5, 1)
    e = torch.where(v == 0, torch.full_like(e, emin + 1), e)
    return 0.5 * torch.exp2(((e - 1).clamp(min=emin) - mant).double())


def _check(g, r, path, guards=(), f32_path=None):
    """g within the bar of `path` of r; a 2-byte g within half an ulp of its type plus the float32 bar of `f32_path` times
    the peak at every element; every gradient of `guards` (a wrong reference) outside the bar."""
    assert bool(torch.isfinite(g).all())
    r = r.detach().double().cpu()
    peak, l2 = _errs(g, r)
    w = WORST.get(path, (0.0, 0.0))
    WORST[path] = (max(w[0], peak), max(w[1], l2))
    assert peak <= BARS[path][0] and l2 <= BARS[path][1], (path, peak, l2)
    if g.dtype in (torch.float16, torch.bfloat16):
        gd = g.detach().double().cpu()
        excess = (gd - r).abs() - _half_ulp(torch.maximum(gd.abs(), r.abs()), g.dtype)
        assert float(excess.max()) <= BARS[f32_path][0] * float(r.abs().max()), "more than one rounding to %s" % g.dtype
    for bad in guards:
        assert not _within(bad, r, path), "the bar of %s does not reject a wrong reference" % path


def _negated_at(coef, j):
    """The fold coefficients with every one of the eight vectors negated at fold position j."""
    out = {k: v.clone() for k, v in coef.items()}
    for v in out.values():
        v[j] = -v[j]
    return out


def _pins(m, C, tier):
    """The tier of the plan and of the adjoint plan (built by the backward that just ran) for C channels."""
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    assert m.tier(C) == tier, ("plan", m.tier(C), tier)
    assert lib.ac_mdct_plan_tier(m._adjoint_plans.get(dev), C) == tier, ("adjoint plan", tier)


def _incoming(shape, gform, gen, dtype, scale):
    """The incoming gradient: dense, the expanded ones of X.sum() (stride 0), or a transposed (non-contiguous) tensor."""
    if gform == "sum":
        return torch.ones((), device="cuda", dtype=dtype).expand(shape)
    if gform == "transposed":
        g = torch.randn(tuple(reversed(shape)), device="cuda", generator=gen, dtype=torch.float64)
        return (scale * g).to(dtype).permute(*reversed(range(len(shape))))
    return (scale * torch.randn(shape, device="cuda", generator=gen, dtype=torch.float64)).to(dtype)


def _run(N, wt, pre, B, K, C, dt, tier, generic, gform="dense", scale_t=1.0, scale_i=1.0, seed=0):
    """Both backwards of one configuration, each against the reference with the sensitivity guards."""
    m = audiocodec_amd.MDCTransformer(N, window_type=wt, compute_dtype=dt, precompute_dtype=pre)
    pdt = np.float32 if pre == torch.float32 else np.float64
    coef = ref.fold_coef(N, wt, pdt)
    gen = torch.Generator(device="cuda").manual_seed(1000 * N + 10 * K + C + seed)
    x = (torch.rand(B, K * N, C, device="cuda", generator=gen, dtype=torch.float64) * 2 - 1).to(dt).requires_grad_(True)
    gX = _incoming((B, K + 1, N, C), gform, gen, dt, scale_t)
    Xv = torch.randn(B, K, N, C, device="cuda", generator=gen, dtype=torch.float64).to(dt).requires_grad_(True)
    gy = _incoming((B, (K + 1) * N, C), gform, gen, dt, scale_i)
    assert gform == "dense" or not (gX.is_contiguous() or gy.is_contiguous())
    force = 1 if generic else 0
    assert _lib.load().ac_set_force_generic(force) == 0
    try:
        m.transform(x).backward(gX)
        m.inverse_transform(Xv).backward(gy)
        torch.cuda.synchronize()
        _pins(m, C, 0 if generic else tier)
    finally:
        _lib.load().ac_set_force_generic(0)
    assert x.grad.dtype == dt and Xv.grad.dtype == dt
    gX64, gy64 = gX.double().cpu(), gy.double().cpu()
    rx = ref.transform_grad(x.cpu(), gX64, coef)
    rX = ref.inverse_grad(Xv.cpu(), gy64, coef)
    if dt == torch.float16:        # the range cases test the library, not float16: the true gradients are normal float16
        for r in (rx, rX):
            assert bool(torch.isfinite(r).all()) and float(r.abs().max()) < 65504
            assert float((r.abs() >= F16_TINY).double().mean()) >= 0.8
    # guards: the first block zeroed, one fold position's coefficients negated, the orthogonal-fold shortcut (rect)
    gx_guards = [rx.clone(), ref.transform_grad(x.cpu(), gX64, _negated_at(coef, N // 4))]
    gx_guards[0][:, :N] = 0
    gX_guards = [rX.clone(), ref.inverse_grad(Xv.cpu(), gy64, _negated_at(coef, N // 4))]
    gX_guards[0][:, 0] = 0
    if _lib.window_id(wt) == _lib.WINDOW_RECT:
        gx_guards.append(ref.inverse_transform(gX64, coef)[:, N:-N] / (4.0 * N))
        gX_guards.append(ref.transform(gy64, coef)[:, 1:-1] * (4.0 * N))
    f32_path = "tier%d" % (0 if generic else tier)
    path = f32_path if dt == torch.float32 else str(dt).split(".")[-1]
    _check(x.grad, rx, path, gx_guards, f32_path)
    _check(Xv.grad, rX, path, gX_guards, f32_path)


def _id(c):
    N, wt, pre, B, K, C, tier = c[:7]
    extra = "-" + c[7] if len(c) > 7 else ""
    return "N%d-%s-pre%s-B%dK%dC%d-tier%d%s" % (N, wt, "32" if pre == torch.float32 else "64", B, K, C, tier, extra)


F64, F32 = torch.float64, torch.float32
# float32: (N, window, precompute, B, K, C, tier of the plan [, incoming-gradient form])
FLOAT32 = [
    # tier 3: the wave-level kernels (one frame per wave at 1024 / 2048; several at 512 / 128 / 64, FOLD4 with four
    # coefficients per fold block for float32-precomputed and rectangular windows)
    (1024, "vorbis", F64, 1, 3, 1, 3), (1024, "vorbis", F64, 2, 33, 2, 3), (2048, "sine", F64, 2, 3, 2, 3),
    (512, "vorbis", F64, 2, 33, 2, 3), (512, "vorbis", F32, 2, 3, 1, 3), (64, "vorbis", F64, 1, 33, 2, 3),
    (128, None, F32, 2, 3, 2, 3), (1024, "vorbis", F64, 2, 3, 2, 3, "sum"),
    # tier 2: compile-time LDS-FFT instances, the channel-team forms at C >= 3
    (960, "vorbis", F64, 1, 3, 1, 2), (960, "sine", F64, 2, 1, 2, 2), (960, "vorbis", F64, 1, 33, 3, 2),
    (960, "vorbis", F64, 2, 3, 6, 2), (1024, "rect", F64, 2, 3, 2, 2), (1024, "vorbis", F64, 1, 3, 3, 2),
    (1024, "vorbis", F64, 2, 3, 6, 2), (4096, "vorbis", F64, 1, 3, 2, 2), (8192, "vorbis", F64, 1, 2, 1, 2),
    (120, "vorbis", F64, 2, 33, 3, 2), (16, "rect", F64, 2, 3, 2, 2), (960, "rect", F32, 1, 3, 2, 2),
    (1024, "sine", F32, 2, 3, 1, 2), (960, "vorbis", F64, 1, 3, 3, 2, "transposed"),
    # tier 1: the run-time forms (filters_n % 4 == 2)
    (30, "vorbis", F64, 2, 3, 1, 1), (90, None, F64, 1, 33, 1, 1),
    # tier 0: O(N^2) (half of N not 5-smooth)
    (34, "vorbis", F64, 2, 3, 2, 0), (8190, "vorbis", F64, 1, 2, 1, 0),
]


@pytest.mark.parametrize("case", range(len(FLOAT32)), ids=[_id(c) for c in FLOAT32])
def test_float32_backward_on_every_tier(case):
    """x.grad of transform and X.grad of inverse_transform in float32 against the reference; every other case runs again
    with the generic kernels forced (ac_set_force_generic), tier 0 for the plan and the adjoint plan."""
    N, wt, pre, B, K, C, tier = FLOAT32[case][:7]
    gform = FLOAT32[case][7] if len(FLOAT32[case]) > 7 else "dense"
    _run(N, wt, pre, B, K, C, F32, tier, False, gform, seed=case)
    if case % 2 == 0:
        _run(N, wt, pre, B, K, C, F32, tier, True, gform, seed=case)


# other dtypes: (N, window, B, K, C, tier of the float32 plan); the forward runs the dtype's own kernels (bfloat16 on the
# wave-level kernels at 1024 / 2048, C <= 2; 2-byte tensors on the 8-byte wave / workgroup forms at 960 and 4096; O(N^2)
# at 34; float64 on the O(N^2) kernels in double up to 4096)
DTYPES = [
    (torch.bfloat16, 1024, "vorbis", 2, 3, 2, 3), (torch.bfloat16, 2048, "sine", 1, 3, 1, 3),
    (torch.bfloat16, 960, "vorbis", 1, 3, 2, 2), (torch.bfloat16, 4096, "vorbis", 1, 2, 1, 2),
    (torch.bfloat16, 34, "rect", 2, 3, 1, 0),
    (torch.float16, 1024, "sine", 2, 3, 2, 3), (torch.float16, 960, "vorbis", 1, 3, 1, 2),
    (torch.float16, 4096, "vorbis", 1, 2, 2, 2), (torch.float16, 34, "vorbis", 2, 3, 2, 0),
    (F64, 1024, "vorbis", 2, 3, 2, 3), (F64, 960, "rect", 1, 3, 3, 2), (F64, 4096, "vorbis", 1, 2, 1, 2),
    (F64, 34, None, 2, 3, 1, 0), (F64, 30, "sine", 1, 33, 1, 1),
]


@pytest.mark.parametrize("case", range(len(DTYPES)),
                         ids=["%s-%s" % (str(c[0]).split(".")[-1], _id(c[1:3] + (F64,) + c[3:])) for c in DTYPES])
def test_other_dtypes_backward(case):
    dt, N, wt, B, K, C, tier = DTYPES[case]
    _run(N, wt, F64, B, K, C, dt, tier, False, seed=case)


# incoming gradients near the ends of float16's range: 1e3 into transform's backward (4N T^T g overflows float16 at these
# sizes), 1e-5 into inverse_transform's (S^T g / 4N falls into float16's subnormals); bfloat16 at 960 (4N not a power of two)
RANGE = [(torch.float16, 1024, "vorbis", 1, 3, 2, 3), (torch.float16, 960, "sine", 2, 3, 1, 2),
         (torch.float16, 4096, "vorbis", 1, 2, 1, 2), (torch.bfloat16, 960, "vorbis", 1, 3, 2, 2)]


@pytest.mark.parametrize("case", range(len(RANGE)),
                         ids=["%s-%s" % (str(c[0]).split(".")[-1], _id(c[1:3] + (F64,) + c[3:])) for c in RANGE])
def test_two_byte_gradients_stay_in_range(case):
    dt, N, wt, B, K, C, tier = RANGE[case]
    _run(N, wt, F64, B, K, C, dt, tier, False, scale_t=1e3, scale_i=1e-5, seed=case)


def test_float64_beyond_4096():
    """float64 at 8192: transform serves it (against the reference), its backward and inverse_transform refuse it with a
    ValueError that names the limit (the float64 synthesis kernel holds 2N doubles of LDS)."""
    N = 8192
    m = audiocodec_amd.MDCTransformer(N, compute_dtype=F64)
    gen = torch.Generator(device="cuda").manual_seed(N)
    x = (torch.rand(1, 2 * N, 1, device="cuda", generator=gen, dtype=F64) * 2 - 1).requires_grad_(True)
    X = m.transform(x)
    Xr = ref.transform(x.detach().cpu(), ref.fold_coef(N, "vorbis"))
    assert float((X.detach().cpu() - Xr).abs().max() / Xr.abs().max()) <= 1e-12
    with pytest.raises(ValueError, match="filters_n = 8192: .* up to 4096"):
        X.sum().backward()
    with pytest.raises(ValueError, match="filters_n = 8192: .* up to 4096"):
        m.inverse_transform(X.detach())
    # the limit is exact: 4096 runs both ways
    m4 = audiocodec_amd.MDCTransformer(4096, compute_dtype=F64)
    x4 = torch.rand(1, 2 * 4096, 1, device="cuda", generator=gen, dtype=F64).requires_grad_(True)
    m4.transform(x4).sum().backward()
    assert bool(torch.isfinite(x4.grad).all()) and m4.inverse_transform(m4.transform(x4.detach())).shape == (1, 4 * 4096, 1)


def test_second_order_backward_raises():
    """The backward runs kernels autograd cannot see: a gradient penalty (create_graph=True) through transform /
    inverse_transform raises instead of silently losing that part."""
    m = audiocodec_amd.MDCTransformer(1024)
    x = torch.rand(1, 3 * 1024, 2, device="cuda").requires_grad_(True)
    (gx,) = torch.autograd.grad(m.transform(x).pow(2).sum(), x, create_graph=True)
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.pow(2).sum().backward()
    Xv = torch.randn(1, 3, 1024, 2, device="cuda").requires_grad_(True)
    (gX,) = torch.autograd.grad(m.inverse_transform(Xv).pow(2).sum(), Xv, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gX.pow(2).sum().backward()
